"""The Muon / NorMuon step of csrc/muon.hip against the fp64 reference of tests/_refs64.py at every grid and tile edge, driven
through the C ABI (paradis_muon_step, paradis_muon_step_d) with an address table built as optim.py builds it.

Cases: tests/_muon_cases.py (CASES; the comment next to a case names the branch of the source it selects).  Every case runs
as Muon and NorMuon, on the exact f32 MFMA products (split = 0) and on the bf16x3 products (split = 1), in two views:
w = 0 (then w_new is the update, one rounding away) and w random with weight decay.

Bounds, per matrix of a stack, e(x) = max|x - x64| / max|x64| with x64 the fp64 reference on the same fp32 inputs:
  * m: element-wise |m_hip - m64| <= 2^-23 (|mu m_old| + |m64|): either rounding of mu m + g, contracted or not;
  * the update (w with w_in = 0), w (w_in != 0) and v:  e_hip <= 1.5 e_cpu + 1e-7  and  e_hip <= 1e-5, where e_cpu is the
    largest e of the fp32 CPU evaluations of the same algorithm: torch.matmul, 16-deep k chunks in order, strictly
    sequential rank-1 updates, and for split = 1 also the CPU emulation of the bf16x3 arithmetic.  "Not less accurate
    than fp32 arithmetic" (tests/test_hip_kernel_edges.py, SURVEY.md 8c iii): any ordinary fp32 order of the same
    products is acceptable, nothing else is.  tests/test_refs64_cpu.py keeps the yardsticks themselves under 1e-5 and
    shows that a fourth-digit typo in one Newton-Schulz coefficient moves the update by more than ten times that.

Memory: w, g, m, v, the decoy tensors behind the other columns of the table and the workspace are carved out of one
buffer with at least 64 words of a bit pattern between neighbours and behind the workspace's last byte; everything but
w, m, v and the workspace must come back bit-unchanged.

MEASURED (MI355X; e_hip / e_cpu, per case the pair closest to its bound over Muon and NorMuon and the members of a stack;
"rest": the stack with a member at rest, "v=0": the first NorMuon step, "device lr": paradis_muon_step_d on 33x31 T3):
  case                          update f32         update bf16x3                 v f32              v bf16x3                 w f32              w bf16x3
  1x40                  1.2e-07 / 2.3e-06    4.5e-07 / 2.6e-06    3.2e-08 / 5.1e-08    5.1e-08 / 5.1e-08    1.7e-08 / 5.4e-08    1.5e-08 / 5.4e-08
  40x1                  1.2e-07 / 2.2e-06    1.5e-07 / 2.3e-06    4.2e-08 / 5.9e-07    6.2e-08 / 5.9e-07    3.6e-08 / 7.3e-08    3.6e-08 / 7.3e-08
  33x31                 5.8e-07 / 1.2e-06    5.5e-07 / 1.2e-06    4.6e-08 / 6.8e-08    4.2e-08 / 6.8e-08    4.7e-08 / 7.1e-08    4.7e-08 / 7.1e-08
  8x20                  2.7e-07 / 6.9e-07    3.5e-07 / 6.9e-07    2.6e-08 / 9.3e-08    3.1e-08 / 9.3e-08    4.5e-08 / 5.7e-08    3.7e-08 / 5.7e-08
  64x64                 8.6e-07 / 1.2e-06    9.7e-07 / 1.2e-06    6.5e-08 / 7.4e-08    1.0e-07 / 1.1e-07    5.8e-08 / 8.8e-08    5.4e-08 / 8.8e-08
  64x96                 1.1e-06 / 1.7e-06    7.5e-07 / 1.7e-06    5.5e-08 / 7.9e-08    6.8e-08 / 7.9e-08    4.4e-08 / 7.0e-08    4.4e-08 / 7.0e-08
  300x256               2.4e-06 / 2.0e-06    1.5e-06 / 2.0e-06    5.4e-08 / 9.1e-08    5.7e-08 / 9.1e-08    5.1e-08 / 7.8e-08    5.0e-08 / 7.6e-08
  513x520               3.4e-06 / 3.8e-06    2.0e-06 / 3.8e-06    1.7e-07 / 1.8e-07    1.3e-07 / 1.8e-07    5.2e-08 / 7.2e-08    4.6e-08 / 7.5e-08
  520x513               2.8e-06 / 2.9e-06    2.0e-06 / 3.0e-06    5.2e-08 / 8.2e-08    5.4e-08 / 8.2e-08    4.6e-08 / 6.8e-08    4.3e-08 / 6.8e-08
  33x31 T3              6.3e-07 / 9.3e-07    5.5e-07 / 7.2e-07    5.3e-08 / 4.4e-08    4.4e-08 / 4.4e-08    5.1e-08 / 6.3e-08    5.3e-08 / 7.1e-08
  64x96 T3              1.4e-06 / 1.5e-06    8.8e-07 / 1.5e-06    6.2e-08 / 6.7e-08    6.2e-08 / 7.9e-08    4.7e-08 / 7.4e-08    4.9e-08 / 8.1e-08
  513x520 T3            3.1e-06 / 3.4e-06    2.5e-06 / 3.8e-06    1.7e-07 / 1.8e-07    1.7e-07 / 2.1e-07    5.2e-08 / 7.2e-08    4.7e-08 / 6.9e-08
  33x31 T3 rest                          -                     -    5.3e-08 / 4.4e-08    4.4e-08 / 4.4e-08    5.1e-08 / 6.3e-08    4.7e-08 / 6.3e-08
  64x96 T3 rest                          -                     -    6.2e-08 / 7.9e-08    6.2e-08 / 7.9e-08    4.5e-08 / 7.2e-08    4.5e-08 / 7.2e-08
  513x520 T3 rest                        -                     -    1.7e-07 / 1.8e-07    1.7e-07 / 2.1e-07    5.2e-08 / 7.2e-08    4.7e-08 / 7.4e-08
  33x31 v=0             5.7e-07 / 1.1e-06    5.9e-07 / 1.1e-06    3.6e-07 / 6.2e-07    4.2e-07 / 6.2e-07                     -                     -
  device lr             6.3e-07 / 9.5e-07    5.3e-07 / 7.4e-07    5.3e-08 / 4.4e-08    4.4e-08 / 4.4e-08    4.8e-08 / 6.8e-08    6.3e-08 / 1.1e-07
Largest e_hip / e_cpu of a single output: 1.22 (v of member 0 of 33x31 T3, 5.3e-8 against 4.4e-8: both under the 1e-7
floor); above the floor 1.16 (update of 300x256, NorMuon, f32 MFMA: 2.36e-6 against 2.03e-6).  Largest e_hip 3.6e-6, largest
e_cpu 4.7e-6 (both the update of member 2 of 513x520 T3).  No case needed a fix in muon.hip or the bgemm path.
With the typo 2.8769 -> 2.8766 compiled into muon.hip all 48 cases of test_step_at_every_edge fail their yardstick.
paradis_bgemm direct: bf16x3 1.5e-7 .. 2.4e-7, f32 MFMA 1.9e-7 .. 3.0e-7 of max|C|; integer operands exact in both.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _muon_cases as C

pytestmark = pytest.mark.gpu
PATTERN = 0x7FC0BEEF          # a quiet NaN: read as data it poisons the result, overwritten it is seen


@pytest.fixture(scope="module")
def L():
    from paradis_model_amd import _lib
    return _lib


class _Arena:
    """named regions of one device buffer, each followed by >= 256 bytes of PATTERN"""

    def __init__(self):
        self.at, self.size = {}, 256

    def add(self, name, nbytes, writable):
        assert nbytes % 4 == 0
        self.at[name] = (self.size, nbytes, writable)
        self.size = (self.size + nbytes + 256 + 255) // 256 * 256

    def build(self):
        self.buf = torch.full((self.size // 4,), PATTERN, dtype=torch.int32, device="cuda").view(torch.uint8)

    def f32(self, name):
        off, nbytes, _ = self.at[name]
        return self.buf[off:off + nbytes].view(torch.float32)

    def ptr(self, name):
        return self.buf.data_ptr() + self.at[name][0]

    def frozen(self):
        """the bytes no kernel may change: a copy with the writable regions blanked"""
        c = self.buf.clone()
        for off, nbytes, writable in self.at.values():
            if writable:
                c[off:off + nbytes] = 0
        return c


class _Stack:
    """T same-shaped matrices in an arena, the address table of optim.py around them.  T = 1: a table of stride 1.
    T = 3: the group sits at columns 2..4 of a table with stride 7 whose other columns hold decoy tensors."""

    def __init__(self, L, rows, cols, T, normuon, w_zero=False, v_zero=False, zero_member=None):
        self.L, self.rows, self.cols, self.T, self.normuon = L, rows, cols, T, normuon
        n = rows * cols
        self.stride, self.first = (1, 0) if T == 1 else (7, 2)
        A = self.A = _Arena()
        for t in range(T):
            A.add(f"w{t}", 4 * n, True)
            A.add(f"g{t}", 4 * n, False)
            A.add(f"m{t}", 4 * n, True)
            if normuon:
                A.add(f"v{t}", 4 * rows, True)
        self.decoys = [c for c in range(self.stride) if not self.first <= c < self.first + T]
        for c in self.decoys:
            for k in "wgm":
                A.add(f"d{k}{c}", 4 * n, False)
            A.add(f"dv{c}", 4 * rows, False)
        self.ws_bytes = int(L.lib.paradis_muon_ws_bytes(T, rows, cols))
        A.add("ws", self.ws_bytes, True)
        A.build()
        self.inp = []
        for t in range(T):
            i = dict(C.inputs(rows, cols, t))
            if w_zero:
                i["w"] = torch.zeros_like(i["w"])
            if v_zero:
                i["v"] = torch.zeros_like(i["v"])
            if t == zero_member:
                i["g"], i["m"] = torch.zeros_like(i["g"]), torch.zeros_like(i["m"])
            self.inp.append(i)
        self.restore()
        gen = torch.Generator(device="cuda").manual_seed(5)
        for c in self.decoys:
            for k in ("dw", "dg", "dm", "dv"):
                r = A.f32(f"{k}{c}")
                r.copy_(torch.rand(r.shape, generator=gen, device="cuda") + 0.5)
        tab = torch.zeros(4, self.stride, dtype=torch.int64)
        for c in self.decoys:
            for row, k in enumerate(("dw", "dg", "dm", "dv")):
                tab[row, c] = A.ptr(f"{k}{c}")
        for t in range(T):
            for row, k in enumerate("wgm"):
                tab[row, self.first + t] = A.ptr(f"{k}{t}")
            tab[3, self.first + t] = A.ptr(f"v{t}") if normuon else 0
        self.tab = tab.cuda()
        self.keep = A.frozen()

    def restore(self):
        """the inputs (again) into w, g, m, v; the workspace is left as it is"""
        for t, i in enumerate(self.inp):
            for k in ("w", "g", "m") + (("v",) if self.normuon else ()):
                self.A.f32(f"{k}{t}").copy_(i[k].reshape(-1))

    def step(self, split, nesterov, lr=C.LR, lr_adj=C.LR_ADJ, dev=None, lr_scale=1.0):
        L = self.L
        tab = ctypes.c_void_p(self.tab.data_ptr() + 8 * self.first)
        head = (tab, self.stride, self.T, self.rows, self.cols, lr, lr_adj, C.MU, C.BETA2, C.WD, C.EPS, int(nesterov),
                int(self.normuon), int(split), ctypes.c_void_p(self.A.ptr("ws")))
        if dev is None:
            rc = L.lib.paradis_muon_step(*head, L.stream_ptr())
        else:
            rc = L.lib.paradis_muon_step_d(*head, L.dptr(dev), lr_scale, L.stream_ptr())
        L.check(rc, "muon_step")
        torch.cuda.synchronize()
        assert torch.equal(self.A.frozen(), self.keep), "a guard word, g or a decoy tensor changed"
        return [{k: self.A.f32(f"{k}{t}").cpu().reshape(self.inp[t][k].shape)
                 for k in ("w", "m") + (("v",) if self.normuon else ())} for t in range(self.T)]


class _Judge:
    """collects e_hip / e_cpu per output, prints and records them, asserts both bounds at the end"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad, self.ratio = record_property, case, [], 0.0

    def add(self, name, got, ref, cpus):
        e_hip, e_cpu = C.err(got, ref), max(C.err(c, ref) for c in cpus)
        print(f"EDGE | {self.case} | {name} | e_hip {e_hip:.2e} | e_cpu {e_cpu:.2e}")
        self.rp(name, f"e_hip={e_hip:.3e} e_cpu={e_cpu:.3e}")
        if not e_hip <= C.CEILING:
            self.bad.append((name, "ceiling", e_hip, C.CEILING))
        if not e_hip <= 1.5 * e_cpu + 1e-7:
            self.bad.append((name, "fp32 yardstick", e_hip, e_cpu))

    def momentum(self, name, got, m64, m_old):
        over = (got.double() - m64).abs() - 2.0 ** -23 * ((C.MU * m_old.double()).abs() + m64.abs())
        if not float(over.max()) <= 0.0:
            self.bad.append((name, "momentum rounding", float(over.max())))

    def done(self):
        assert not self.bad, (self.case, self.bad)


def _judge_member(J, tag, out, inp, r, split, normuon, update):
    cpus = [r["cpu"][o] for o in C.orders_of(split)]
    J.momentum(f"{tag} m", out["m"], r["m64"], inp["m"])
    J.add(f"{tag} {'update' if update else 'w'}", out["w"], r["w64"], [c[0] for c in cpus])
    if normuon:
        J.add(f"{tag} v", out["v"], r["v64"], [c[1] for c in cpus])


def _both_views(L, J, name, normuon, split, **step_kw):
    """the case in the two views; returns nothing, J holds the verdicts"""
    _, rows, cols, T, nesterov = C.CASE[name]
    ref_kw = {k: step_kw[k] for k in ("lr", "lr_adj") if k in step_kw}
    call_kw = dict(step_kw)
    if "dev" in call_kw:          # the device state's learning rate is the one that counts: the host's are decoys
        call_kw.update(lr=123.0, lr_adj=456.0)
    first = None
    for w_zero in (True, False):
        S = _Stack(L, rows, cols, T, normuon, w_zero=w_zero)
        outs = S.step(split, nesterov, **call_kw)
        for t in range(T):
            r = C.refs(rows, cols, t, nesterov, normuon, w_zero=w_zero, **ref_kw)
            _judge_member(J, f"t{t} {'w=0' if w_zero else 'decay'}", outs[t], S.inp[t], r, split, normuon, w_zero)
        if first is None:
            first = outs
        else:             # m and v do not depend on w: the same bits in both views (fixed-order sums)
            for a, b in zip(first, outs):
                assert torch.equal(a["m"], b["m"]) and (not normuon or torch.equal(a["v"], b["v"]))
        del S


FAMILIES = [pytest.param(False, id="muon"), pytest.param(True, id="normuon")]
SPLITS = [pytest.param(0, id="f32"), pytest.param(1, id="bf16x3")]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("normuon", FAMILIES)
@pytest.mark.parametrize("name", [c[0] for c in C.CASES])
def test_step_at_every_edge(L, record_property, name, normuon, split):
    J = _Judge(record_property, f"{name} {'normuon' if normuon else 'muon'} split{split}")
    _both_views(L, J, name, normuon, split)
    J.done()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("normuon", FAMILIES)
@pytest.mark.parametrize("name", ["33x31 T3", "64x96 T3", "513x520 T3"])
def test_stack_with_a_member_at_rest(L, record_property, name, normuon, split):
    """Member 1 of the stack has zero gradient and zero momentum: its w comes back as exactly w * decay, its m as zeros, its v
    as beta2 v to one fp32 rounding; its neighbours as in the plain stack."""
    _, rows, cols, T, nesterov = C.CASE[name]
    J = _Judge(record_property, f"{name} rest {'normuon' if normuon else 'muon'} split{split}")
    S = _Stack(L, rows, cols, T, normuon, zero_member=1)
    outs = S.step(split, nesterov)
    for t in (0, 2):
        _judge_member(J, f"t{t} decay", outs[t], S.inp[t], C.refs(rows, cols, t, nesterov, normuon, w_zero=False), split,
                      normuon, False)
    decay = np.float32(1) - np.float32(C.LR) * np.float32(C.WD)
    assert torch.equal(outs[1]["w"], torch.from_numpy(S.inp[1]["w"].numpy() * decay))
    assert torch.equal(outs[1]["m"], torch.zeros(rows, cols)) and not bool(torch.signbit(outs[1]["m"]).any())
    if normuon:
        want = C.BETA2 * S.inp[1]["v"].double()
        assert bool(((outs[1]["v"].double() - want).abs() <= 2.0 ** -24 * want).all())
    J.done()


@pytest.mark.parametrize("split", SPLITS)
def test_first_normuon_step(L, record_property, split):
    """v = 0 going in: the first step of a run"""
    name = "33x31"
    _, rows, cols, T, nesterov = C.CASE[name]
    J = _Judge(record_property, f"{name} first step split{split}")
    S = _Stack(L, rows, cols, T, True, w_zero=True, v_zero=True)
    out = S.step(split, nesterov)[0]
    _judge_member(J, "t0 w=0", out, S.inp[0], C.refs(rows, cols, 0, nesterov, True, w_zero=True, v_zero=True), split, True, True)
    J.done()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("normuon", FAMILIES)
def test_device_learning_rate(L, record_property, normuon, split):
    """paradis_muon_step_d: lr from the device state, lr_adj = fp32(lr * lr_scale) formed in the kernel; the host's lr and
    lr_adj arguments are not used."""
    lr, scale = C.f32(3e-3), 7.3
    dev = torch.tensor([11, int(np.float32(lr).view(np.int32))], dtype=torch.int32).cuda()
    J = _Judge(record_property, f"device lr {'normuon' if normuon else 'muon'} split{split}")
    _both_views(L, J, "33x31 T3", normuon, split, lr=lr, lr_adj=C.f32(lr * scale), dev=dev, lr_scale=scale)
    assert dev.cpu().tolist() == [11, int(np.float32(lr).view(np.int32))]
    J.done()


@pytest.mark.parametrize("split", SPLITS)
def test_zero_adjusted_rate_is_pure_decay(L, split):
    """lr_adj = 0, Muon: w_new = fp32(w * fp32(1 - fp32(lr * wd))) bit for bit"""
    _, rows, cols, T, nesterov = C.CASE["33x31"]
    S = _Stack(L, rows, cols, T, False)
    out = S.step(split, nesterov, lr_adj=0.0)[0]
    decay = np.float32(1) - np.float32(C.LR) * np.float32(C.WD)
    assert torch.equal(out["w"], torch.from_numpy(S.inp[0]["w"].numpy() * decay))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("normuon", FAMILIES)
@pytest.mark.parametrize("rows,cols", [(300, 256), (513, 520)])
def test_two_identical_steps_give_identical_bits(L, rows, cols, normuon, split):
    """The norm sums are reduced in a fixed order (muon.hip, block_sum_fixed): the same inputs give the same bits in w, m
    and v, T = 3.  The second call finds the workspace as the first one left it."""
    S = _Stack(L, rows, cols, 3, normuon)
    a = S.step(split, True)
    S.restore()
    b = S.step(split, True)
    for x, y in zip(a, b):
        for k in x:
            assert torch.equal(x[k], y[k]), k
            assert bool(torch.isfinite(x[k]).all())


# ================================================================================================ paradis_bgemm
# The Newton-Schulz products directly, with the transposed left operand supplied (AT: the LDS-DMA exact kernel can run)
# and batch strides larger than the matrices, as the step's 64-word aligned buffers have.
BGEMM = [  # M, K, N, words added to every batch stride, words the operand bases are moved by
    (132, 48, 260, 64, 0),    # eligible (pd_exact_dma_eligible): LDS-DMA kernel, ragged 128 x 128 tiles both ways
    (132, 40, 260, 64, 0),    # K % 16 != 0: register-staged kernel
    (130, 48, 260, 64, 0),    # M % 4 != 0
    (132, 48, 258, 64, 0),    # N % 4 != 0
    (132, 48, 260, 66, 0),    # batch strides % 4 != 0
    (132, 48, 260, 64, 1),    # a 4-byte aligned view of every operand
]


def _strided(mats, pad, shift, fill):
    """the [nb, r, c] matrices at batch stride r * c + pad behind `shift` words, `fill` everywhere else"""
    nb, r, c = mats.shape
    bs = r * c + pad
    buf = torch.full((shift + nb * bs,), fill, dtype=torch.float32, device="cuda")
    view = buf[shift:].view(nb, bs)
    view[:, :r * c] = mats.reshape(nb, -1).cuda()
    return buf, view, bs


def _bgemm(L, A, B, pad, shift, split):
    nb, M, K = A.shape
    N = B.shape[2]
    nan = float("nan")
    a_buf, a_v, a_bs = _strided(A, pad, shift, nan)
    at_buf, at_v, at_bs = _strided(A.mT.contiguous(), pad, shift, nan)
    b_buf, b_v, b_bs = _strided(B, pad, shift, nan)
    c_buf, c_v, c_bs = _strided(torch.zeros(nb, M, N), pad, shift, 0.0)
    c_buf.view(torch.int32).fill_(PATTERN)
    ws = torch.empty(nb * L.lib.paradis_pw_gemm_split_bytes(M, K, 3), dtype=torch.uint8, device="cuda") if split else None
    L.check(L.lib.paradis_bgemm(L.dptr(a_v), L.dptr(at_v), L.dptr(b_v), L.dptr(c_v), nb, M, K, N, a_bs, at_bs, b_bs, c_bs,
                                L.dptr(ws), L.stream_ptr()), "bgemm")
    torch.cuda.synchronize()
    out = c_v[:, :M * N].reshape(nb, M, N).cpu()
    gaps = torch.cat([c_buf[:shift], c_v[:, M * N:].reshape(-1)]).view(torch.int32)
    assert bool((gaps == PATTERN).all()), "bgemm wrote between the matrices of C"
    return out


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("M,K,N,pad,shift", BGEMM)
def test_bgemm_with_transposed_operand_and_batch_strides(L, record_property, M, K, N, pad, shift, nb):
    g = torch.Generator().manual_seed(M + K + N + pad + shift + nb)
    A, B = torch.randn(nb, M, K, generator=g) * K ** -0.5, torch.randn(nb, K, N, generator=g)
    ref = A.double() @ B.double()
    errs = {split: C.err(_bgemm(L, A, B, pad, shift, split), ref) for split in (0, 1)}
    print(f"EDGE | bgemm {M}x{K}x{N} pad{pad} shift{shift} nb{nb} | C | split {errs[1]:.2e} | exact {errs[0]:.2e}")
    record_property("C", f"e_split={errs[1]:.3e} e_exact={errs[0]:.3e}")
    # the bounds of test_batched_gemm_split_vs_exact (tests/test_hip_gemm_split.py), and its 2e-6 for the exact kernel too
    assert errs[1] <= 1.25 * errs[0] + 1e-7 and errs[1] <= 2e-6 and errs[0] <= 2e-6, errs
    # small integers: every product and partial sum is exact in both arithmetics
    A, B = torch.randint(-8, 9, (nb, M, K), generator=g).float(), torch.randint(-8, 9, (nb, K, N), generator=g).float()
    ref = A.double() @ B.double()
    for split in (0, 1):
        assert torch.equal(_bgemm(L, A, B, pad, shift, split).double(), ref), split
