"""The small streaming / reduction kernels against plain fp64 references (tests/_refs64.py) at every dispatch edge:
the shapes, alignments and sizes at which csrc/resample.hip, gbias.hip, elementwise.hip, norm.hip and train.hip pick another kernel,
another chunk count or another tail loop.  The parameter lists are derived from the dispatch conditions in the source;
the comment next to a case names the branch it selects.

For every output      e_hip = max|hip - ref64| / max|ref64|      and e_cpu, the same for an fp32 CPU evaluation
(the oracle, or plain ATen).  Asserted: (1) the project's ceilings (SURVEY.md 8c ii: 1e-5 forward, 1e-4 gradients; 1e-6
AdamW) and (2) "not less accurate than fp32 arithmetic": e_hip <= 1.5 e_cpu + 1e-7 (SURVEY.md 8c iii; the floor of
test_split_not_less_accurate_than_exact_f32).  For sums over >= 256 terms e_cpu is the larger of torch.sum's error and
that of a strictly sequential fp32 accumulation of the same fp32 terms (numpy.cumsum in float32): the least favourable
ordinary order, measured on the reference side only.  Every figure is printed (``-s``) and recorded as a property.

Input design: the first and last element of each reduced range and the last element in front of each chunk / tile
boundary of the source are 2^10 times the rest, so a dropped or doubled one is seen; at least one case per kernel has
strictly positive terms, so nothing cancels.

The weight gradient of the pointwise GEMMs closes the file: one call per kernel its plan (csrc/gemm_common.h, wgrad_plan)
can choose, on integer-valued operands, against fp64 with tolerance zero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import paradis_oracle as O
from tests import _refs64 as R

pytestmark = pytest.mark.gpu
FWD, BWD, ADAM = 1e-5, 1e-4, 1e-6
SPIKE = 1024.0


@pytest.fixture(scope="module")
def ops():
    from paradis_model_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from paradis_model_amd import _lib
    return _lib


def _rand(seed, *shape, positive=False, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if positive:
        return (torch.rand(*shape, generator=g, device="cuda") + 0.5) * scale
    return torch.randn(*shape, generator=g, device="cuda") * scale


def _spike(t, dim, idx):
    """t[..., i, ...] *= 2^10 for the valid, distinct i of idx along dim"""
    n = t.shape[dim]
    ok = sorted({i % n for i in idx if -n <= i < n})
    t.index_copy_(dim, torch.tensor(ok, device=t.device), t.index_select(dim, torch.tensor(ok, device=t.device)) * SPIKE)
    return t


def _spike_cross(t, dim_a, idx_a, dim_b, idx_b):
    """t *= 2^10 where the index along dim_a is in idx_a AND the one along dim_b is in idx_b: the ends of a second
    reduced axis, at a few positions of the first only (whole slices would set the scale of the output by themselves)"""
    na, nb = t.shape[dim_a], t.shape[dim_b]
    ia = torch.tensor(sorted({i % na for i in idx_a if -na <= i < na}), device=t.device)
    ib = torch.tensor(sorted({i % nb for i in idx_b if -nb <= i < nb}), device=t.device)
    sub = t.index_select(dim_a, ia)
    sub.index_copy_(dim_b, ib, sub.index_select(dim_b, ib) * SPIKE)
    t.index_copy_(dim_a, ia, sub)
    return t


def _corners(t):
    """the four corners of every plane (pole rows x wrap columns) *= 2^10"""
    return _spike_cross(t, -2, [0, -1], -1, [0, -1])


def _e(got, ref):
    ref = ref.detach()
    got = got.detach().to(ref.device).double().reshape(ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _seq_sum(terms):
    """strictly sequential fp32 sum over the last axis of an fp32 CPU tensor"""
    a = np.ascontiguousarray(terms.detach().cpu().numpy().astype(np.float32, copy=False))
    return torch.from_numpy(np.cumsum(a, axis=-1, dtype=np.float32)[..., -1].copy())


class _Judge:
    """collects e_hip / e_cpu per output, prints and records them, asserts both bounds at the end"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad = record_property, case, []

    def add(self, name, got, ref, cpu, ceil, seq=None):
        e_hip, e_cpu = _e(got, ref), _e(cpu, ref)
        if seq is not None:
            e_cpu = max(e_cpu, _e(seq, ref))
        print(f"EDGE | {self.case} | {name} | e_hip {e_hip:.2e} | e_cpu {e_cpu:.2e}")
        self.rp(name, f"e_hip={e_hip:.3e} e_cpu={e_cpu:.3e}")
        if not e_hip <= ceil:
            self.bad.append((name, "ceiling", e_hip, ceil))
        if not e_hip <= 1.5 * e_cpu + 1e-7:
            self.bad.append((name, "fp32 yardstick", e_hip, e_cpu))

    def done(self):
        assert not self.bad, (self.case, self.bad)


def _leaf64(t):
    return t.detach().double().clone().requires_grad_(True)


def _leaf32(t):
    return t.detach().cpu().clone().requires_grad_(True)


# ================================================================================================ avgpool
# resample.hip: one thread per output (forward) / per input cell (backward, a gather over the windows [o s, o s + 4] of
# the padded plane that hold an alias of the cell); grid-stride loop above 8192 workgroups (721x1440: 4056 - below);
# strides 5: windows abut; 7: they leave rows / columns uncovered; 3, 5, 7 do not divide H - 1 or W of most grids.
POOL_GRIDS = [(12, 16), (13, 16),
              (9, 4),            # W = 4: every column has an alias in the halo (jb >= W - p and jb < p together cover all)
              (33, 64), (32, 64), (128, 256),
              (721, 1440)]       # one plane of the production grid


@pytest.mark.parametrize("H,W", POOL_GRIDS)
@pytest.mark.parametrize("s", [1, 2, 3, 4, 5, 7])
def test_avgpool_geo(ops, record_property, H, W, s):
    planes = (1, 1) if H * W > 100000 else (2, 3)
    positive = (s + H) % 2 == 0                       # half of the cases: strictly positive terms
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, gy = _rand(1, *planes, H, W, positive=positive), _rand(2, *planes, Ho, Wo, positive=positive)
    for t in (x, gy):                                 # the plane's corners: pole rows, wrap columns
        _corners(t)
    J = _Judge(record_property, f"avgpool {H}x{W} s{s}")
    y = ops._avgpool_geo(x, s)
    gx = ops._avgpool_geo_backward(gy, H, W, s)
    assert torch.equal(gx, ops._avgpool_geo_backward(gy, H, W, s))      # a gather: no atomics
    xr, xc = _leaf64(x), _leaf32(x)
    yr, yc = R.avgpool_geo(xr, s), O.avgpool_geo(xc, s)
    assert tuple(y.shape) == tuple(yr.shape)
    yr.backward(gy.double())
    yc.backward(gy.cpu())
    J.add("y", y, yr, yc, FWD)
    J.add("gx", gx, xr.grad, xc.grad, BWD)
    if s >= 6:       # cells no window covers: exactly zero gradient (found on the reference side with a positive cotangent)
        probe = torch.zeros(1, 1, H, W, dtype=torch.float64, device="cuda", requires_grad=True)
        R.avgpool_geo(probe, s).sum().backward()
        uncovered = probe.grad[0, 0] == 0
        assert bool(uncovered.any()) and bool((gx[:, :, uncovered] == 0).all())
    if s == 1 and W >= 8:      # what the model runs at stride 1: the depthwise stencil with uniform taps
        xd = x.clone().requires_grad_(True)
        y1 = ops.avgpool_geo(xd, 1)
        y1.backward(gy)
        J.add("y (stencil route)", y1, yr, yc, FWD)
        J.add("gx (stencil route)", xd.grad, xr.grad, xc.grad, BWD)
    J.done()


def test_avgpool_geo_rejects_what_the_header_excludes(L):
    """include/paradis_hip.h (a11): H >= 4 and W >= 4, W even - rc 1, nothing launched"""
    x = torch.zeros(64, device="cuda")
    for H, W in ((3, 8), (8, 2), (8, 5)):
        assert L.lib.paradis_avgpool_geo_fwd(L.dptr(x), L.dptr(x), 1, H, W, 2, L.stream_ptr()) == 1
        assert L.lib.paradis_avgpool_geo_bwd(L.dptr(x), L.dptr(x), 1, H, W, 2, L.stream_ptr()) == 1
    assert L.lib.paradis_avgpool_geo_fwd(L.dptr(x), L.dptr(x), 1, 8, 8, 0, L.stream_ptr()) == 1


@pytest.mark.parametrize("Hc,Wc,H,W", [(9, 16, 33, 64), (16, 32, 32, 64), (5, 7, 5, 28),
                                       (181, 360, 721, 1440)])       # one plane of the production grid, stride 4
def test_upsample_lonp(ops, record_property, Hc, Wc, H, W):
    x, gy = _rand(1, 1, 2, Hc, Wc), _rand(2, 1, 2, H, W, positive=True)
    for t in (x, gy):
        _corners(t)
    J = _Judge(record_property, f"upsample {Hc}x{Wc}->{H}x{W}")
    y = ops._upsample_lonp(x, H, W)
    gx = ops._upsample_lonp_backward(gy, Hc, Wc)
    assert torch.equal(gx, ops._upsample_lonp_backward(gy, Hc, Wc))     # documented atomic-free
    xr, xc = _leaf64(x), _leaf32(x)
    yr, yc = R.upsample_lonp(xr, H, W), O.upsample_lon_periodic(xc, H, W)
    yr.backward(gy.double())
    yc.backward(gy.cpu())
    J.add("y", y, yr, yc, FWD)
    J.add("gx", gx, xr.grad, xc.grad, BWD)
    J.done()


# ================================================================================================ global bias
def _rank_spikes(Rk):
    """rank indices in front of the quarter split rq = ceil(R / 4) of gbias_m8_*_kernel and of its batches of 8"""
    rq = (Rk + 3) // 4
    return [0, Rk - 1, rq - 1, 2 * rq - 1, 3 * rq - 1, 7, 8]


def _gbias_inputs(Cin, Co, Rk, H, W, positive):
    A = _spike(_rand(1, Cin, Rk, positive=positive, scale=0.5), 1, _rank_spikes(Rk))
    U, V = _rand(2, Rk, H, positive=positive), _rand(3, Rk, W, positive=positive)
    Pw = _spike(_rand(4, Co, Cin, positive=positive, scale=0.5), 1, [0, -1]) if Co else None
    return A, U, V, Pw


GB_FWD = [
    # (Cin, Co, R, H, W): H W < 2^17 -> gbias_m8_kernel (one row per workgroup), rank range in four quarters
    (8, None, 16, 12, 16), (8, 24, 1, 12, 16), (8, 24, 3, 12, 16),       # R < 4: empty quarters
    (8, 24, 5, 12, 16), (8, 24, 16, 12, 16), (8, 24, 30, 12, 16),       # R % 4, R % 8 != 0: scalar rank tail
    (3, 7, 5, 9, 4), (17, 20, 30, 33, 64), (5, 8, 7, 40, 300),          # W < 64, = 64, > 256 (ragged last column tile)
    # H W >= 2^17 and R <= 256 -> gbias_m8_rows_kernel<8>; H = 721: last row tile holds one row
    (2, None, 1, 721, 1440), (2, None, 3, 721, 1440), (2, None, 5, 721, 1440), (2, None, 30, 721, 1440),
    (8, 4, 16, 721, 1440),
    (8, 1024, 16, 256, 512),     # exactly 2^17 pixels, Co = 1024 (small_mix_kernel, 1024 output rows)
    (1, None, 256, 256, 512),    # R = GM8_MAXR: the largest coefficient table
    (1, None, 257, 256, 512),    # R > GM8_MAXR: falls back to the one-row kernel
]


@pytest.mark.parametrize("Cin,Co,Rk,H,W", GB_FWD)
def test_global_bias_forward(ops, record_property, Cin, Co, Rk, H, W):
    positive = Rk % 2 == 1
    A, U, V, Pw = _gbias_inputs(Cin, Co, Rk, H, W, positive)
    J = _Judge(record_property, f"gbias fwd Cin{Cin} Co{Co} R{Rk} {H}x{W}")
    out, m8 = ops._global_bias_map(A, U, V, Pw)
    ref_m8 = R.global_bias_m8(A.double(), U.double(), V.double())
    cpu_m8 = O.global_bias_map(A.cpu(), U.cpu(), V.cpu(), None)
    seq = None
    if Rk >= 256:       # a sum over >= 256 terms: the sequential yardstick over the same fp32 products (a u) v
        t = (A.cpu()[:, None, None, :] * U.cpu().t()[None, :, None, :]) * V.cpu().t()[None, None, :, :]
        seq = _seq_sum(t)
    J.add("m8", m8 if Co else out, ref_m8, cpu_m8, FWD, seq)
    if Co:
        J.add("map", out, R.global_bias_map(A.double(), U.double(), V.double(), Pw.double()),
              O.global_bias_map(A.cpu(), U.cpu(), V.cpu(), Pw.cpu()), FWD)
    J.done()


def _gbias_seq(gmap_c, A_c, U_c, V_c, Pw_c):
    """sequential-order yardsticks of the sums over >= 256 terms (gPw over the pixels, gA over the plane, gU / gV on the
    larger grids) from fp32 CPU terms"""
    Cin = A_c.shape[0]
    m8 = O.global_bias_map(A_c, U_c, V_c, None).reshape(Cin, -1)
    g = gmap_c.reshape(gmap_c.shape[0], -1)
    seq_pw = _seq_sum(g[:, None, :] * m8[None, :, :]) if Pw_c is not None and g.shape[1] >= 256 else None
    gm8 = (Pw_c.t() @ g) if Pw_c is not None else g
    uv = (U_c[:, :, None] * V_c[:, None, :]).reshape(U_c.shape[0], -1)           # [R, P]
    seq = {"Pw": seq_pw, "A": _seq_sum(gm8[:, None, :] * uv[None, :, :])}
    # gU[r,h] sums Cin W terms, gV[r,w] Cin H terms: the same yardstick wherever that is >= 256
    H, W = U_c.shape[1], V_c.shape[1]
    t = gm8.reshape(Cin, 1, H, W) * A_c[:, :, None, None]                       # [Cin, R, H, W]
    if Cin * W >= 256:
        seq["U"] = _seq_sum((t * V_c[None, :, None, :]).permute(1, 2, 0, 3).reshape(-1, H, Cin * W))
    if Cin * H >= 256:
        seq["V"] = _seq_sum((t * U_c[None, :, :, None]).permute(1, 3, 0, 2).reshape(-1, W, Cin * H))
    return seq


@pytest.mark.parametrize("Cin", [3, 8,      # Cin <= 8: gbias_gm8_kernel<8>; gPw by gbias_gpw_rows_kernel<2,8> at P >= 2048, P % 4 == 0
                                 9, 16,     # 8 < Cin <= 16: gbias_gm8_kernel<16>, gPw by gbias_gpw_kernel
                                 17])       # Cin > 16: small_mix_kernel forms gm8
@pytest.mark.parametrize("H,W,Co", [(97, 40, 24),      # P = 3880 >= 2048; H > 64: the wave loop of gbias_finish_kernel runs twice
                                    (12, 16, 24),      # P < 2048: gbias_gpw_kernel for every Cin
                                    (97, 40, None)])   # no projection: gA / gU / gV straight from gmap
def test_global_bias_map_backward(ops, record_property, Cin, H, W, Co):
    Rk, positive = 6, Cin in (8, 17)
    A, U, V, Pw = _gbias_inputs(Cin, Co, Rk, H, W, positive)
    gmap = _rand(5, Co or Cin, H, W, positive=positive)
    g2 = gmap.view(gmap.shape[0], -1)
    _spike(g2, 1, [0, -1, 1023, 1024, 63, 255])                   # ends of the pixel range and of its 256-wide strides
    _spike_cross(g2, 0, [0, -1, 15, 16], 1, [5, -7])              # ends of the sum over Co (gm8), at two pixels
    names = ["A", "U", "V"] + (["Pw"] if Co else [])
    J = _Judge(record_property, f"gbias bwd Cin{Cin} Co{Co} {H}x{W}")
    runs = []
    for _ in range(2):
        lv = [t.clone().requires_grad_(True) for t in (A, U, V, Pw) if t is not None]
        ops.global_bias_map(*lv).backward(gmap)
        runs.append([t.grad for t in lv])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                       # no atomics anywhere in this backward
    lr = [_leaf64(t) for t in (A, U, V, Pw) if t is not None]
    R.global_bias_map(*lr).backward(gmap.double())
    lc = [_leaf32(t) for t in (A, U, V, Pw) if t is not None]
    O.global_bias_map(*lc, *(() if Co else (None,))).backward(gmap.cpu())
    seqs = _gbias_seq(gmap.cpu(), A.cpu(), U.cpu(), V.cpu(), Pw.cpu() if Co else None)
    for n, got, r, c in zip(names, runs[0], lr, lc):
        J.add("g" + n, got, r.grad, c.grad, BWD, seqs.get(n) if H * W >= 256 else None)
    J.done()


@pytest.mark.parametrize("Co", [7,          # gbias_gpw_rows_kernel<2,8>, last workgroup holds one row
                                1023,       # ... the same below the 1024 switch
                                1025])      # gbias_gpw_rows_kernel<4,8>, Co % 4 == 1
@pytest.mark.parametrize("H,W", [(28, 73),      # P = 2044 < 2048: gbias_gpw_kernel
                                 (32, 64),      # P = 2048: the rows kernels
                                 (25, 82)])     # P = 2050, P % 4 == 2: gbias_gpw_kernel
def test_global_bias_m8_and_fused_projection_backward(ops, record_property, Co, H, W):
    """The backward of ``pointwise(..., bias_proj=(global_bias_m8(A, U, V), Pw))`` without its GEMM (which has its own
    file): paradis_global_bias_proj_bwd on the cotangent of the map, then paradis_global_bias_m8_bwd."""
    Cin, Rk, positive = 8, 6, Co == 1023
    A, U, V, Pw = _gbias_inputs(Cin, Co, Rk, H, W, positive)
    gmap = _rand(5, Co, H, W, positive=positive)
    g2 = gmap.view(Co, -1)
    _spike(g2, 1, [0, -1, 1023, 1024, 2043, 2047])                # ends of the pixel range and of its 256-float4 strides
    per = (Co + 15) // 16                                         # gbias_gm8_kernel: 16 slices of `per` rows of Co
    _spike_cross(g2, 0, [0, -1, Co - 2, per - 1, per, 15 * per - 1], 1, [5, -7])
    J = _Judge(record_property, f"gbias m8+proj bwd Co{Co} {H}x{W}")
    runs = []
    for _ in range(2):
        lv = [t.clone().requires_grad_(True) for t in (A, U, V)]
        m8 = ops.global_bias_m8(*lv)
        gpw, gm8 = ops._global_bias_proj_backward(gmap, m8.detach(), Pw)
        m8.backward(gm8)
        runs.append([t.grad for t in lv] + [gpw, gm8])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                       # gm8: slices summed in LDS in slice order (documented atomic-free)
    lr, lc = [_leaf64(t) for t in (A, U, V, Pw)], [_leaf32(t) for t in (A, U, V, Pw)]
    R.global_bias_map(*lr).backward(gmap.double())
    O.global_bias_map(*lc).backward(gmap.cpu())
    seqs = _gbias_seq(gmap.cpu(), A.cpu(), U.cpu(), V.cpu(), Pw.cpu())
    J.add("gm8", runs[0][4], (Pw.double().t() @ gmap.double().view(Co, -1)), (Pw.cpu().t() @ gmap.cpu().view(Co, -1)), BWD,
          _seq_sum((Pw.cpu().t()[:, None, :] * gmap.cpu().view(Co, -1).t()[None, :, :])) if Co >= 256 else None)
    gpu_order = {"A": 0, "U": 1, "V": 2, "Pw": 3}
    for i, n in enumerate(("A", "U", "V", "Pw")):
        J.add("g" + n, runs[0][gpu_order[n]], lr[i].grad, lc[i].grad, BWD, seqs.get(n))
    J.done()


def test_global_bias_proj_bwd_unaligned_gmap(L, record_property):
    """gmap 4 bytes off a 16-byte boundary through the C ABI: launch_gpw leaves the float4 rows kernel for
    gbias_gpw_kernel; same values as the aligned call up to the summation order, both against fp64."""
    Cin, Co, P = 8, 16, 2048
    m8, Pw = _rand(1, Cin, P), _rand(2, Co, Cin, scale=0.5)
    vals = _spike(_rand(3, Co, P, positive=True), 1, [0, -1, 1023, 1024])
    buf = torch.zeros(Co * P + 8, device="cuda")
    J = _Judge(record_property, "gbias proj bwd unaligned")
    ref_pw = vals.double() @ m8.double().t()
    ref_m8 = Pw.double().t() @ vals.double()
    cpu_pw, cpu_m8 = vals.cpu() @ m8.cpu().t(), Pw.cpu().t() @ vals.cpu()
    seq_pw = _seq_sum(vals.cpu()[:, None, :] * m8.cpu()[None, :, :])
    for off in (0, 1):
        gmap = buf[off:off + Co * P].view(Co, P)
        gmap.copy_(vals)
        assert (gmap.data_ptr() % 16 == 0) == (off == 0)
        gpw, gm8 = torch.full((Co, Cin), -7.0, device="cuda"), torch.full((Cin, P), -7.0, device="cuda")
        rc = L.lib.paradis_global_bias_proj_bwd(L.dptr(gmap), L.dptr(m8), L.dptr(Pw), L.dptr(gpw), L.dptr(gm8), Cin, Co, P,
                                                L.stream_ptr())
        assert rc == 0, L.last_error()
        J.add(f"gPw off{off}", gpw, ref_pw, cpu_pw, BWD, seq_pw)
        J.add(f"gm8 off{off}", gm8, ref_m8, cpu_m8, BWD)
    # Cin > 16 has no kernel on this entry point: rejected, not approximated
    assert L.lib.paradis_global_bias_proj_bwd(L.dptr(buf), L.dptr(m8), L.dptr(Pw), L.dptr(buf), L.dptr(buf), 17, Co, P,
                                              L.stream_ptr()) == 1
    J.done()


# ================================================================================================ channel norm, backward
# norm.hip streaming path: stats kernel (64-pixel tiles), then one apply workgroup per (b, c, chunk of APPLY_SPAN = 8192
# pixels); float4 instantiation when P % 4 == 0 and every slice is 16-byte aligned, scalar otherwise
NORM_P = [8192,               # one chunk, exactly full
          8196,               # two chunks, the second holds ONE float4
          8192 * 2 + 36,      # three apply chunks, ragged last, vec path
          8191,               # one chunk, scalar instantiation (P % 4 == 3), ragged 64-pixel stats tile
          16387]              # three chunks, scalar instantiation, last chunk of 3 pixels
NORM_CASES = [(20, 0, P, add, False) for P in NORM_P for add in (False, True)]
NORM_CASES += [(1024, 128, P, i % 2 == 0, False) for i, P in enumerate(NORM_P)]     # the reaction block's virtual concat
NORM_CASES += [(20, 0, 8196, False, True), (20, 0, 16387, True, True)]              # channel mean >> channel spread
NORM_CASES = [pytest.param(3 if c[0] == 20 else 1, *c, id="-".join(map(str, c))) for c in NORM_CASES]
# the parameter gradients' two-level reduction (norm_bwd_plan: FINISH_ROWS = 64 rows of `partial` per finish chunk, one row
# per (sample, apply chunk)) with more than one finish chunk: B * ceil(P / 8192) > 64
NORM_CASES += [pytest.param(65, 20, 0, 100, False, False, id="B65-20-0-100-False-False"),     # float4, two chunks, the second holds ONE row
               pytest.param(130, 6, 0, 7, False, False, id="B130-6-0-7-False-False"),        # scalar, three chunks (64, 64, 2), ragged stats tile
               pytest.param(65, 20, 12, 100, True, False, id="B65-20-12-100-True-False")]     # virtual concat, with addend


@pytest.mark.parametrize("B,C1,C2,P,add,badly_conditioned", NORM_CASES)
def test_channel_norm_backward(ops, record_property, B, C1, C2, P, add, badly_conditioned):
    """``badly_conditioned``: x = 100 + 0.01 randn per pixel, so x - mean cancels four of fp32's seven digits.  Centred on
    the fp32 mean alone (the reference module's arithmetic, and the kernels' until this test) every fp32 evaluation is
    1e-3 off there: y 9.2e-4, gx 3.6e-4, gw 1.5e-3 from the kernels against 9.7e-4, 2.4e-4, 1.1e-3 from the CPU oracle.
    The kernels now carry the mean's rounding residual (csrc/norm.hip, file header): 2.0e-7, 1.0e-7, 1.2e-7."""
    C = C1 + C2
    positive = P % 2 == 1
    if badly_conditioned:
        x = 100.0 + 0.01 * _rand(1, B, C, 1, P)
    else:
        x = _rand(1, B, C, 1, P, scale=3.0) + 1.0
    x1, x2 = x[:, :C1].contiguous(), (x[:, C1:].contiguous() if C2 else None)
    w, b = 1.0 + _rand(2, C, scale=0.2), _rand(3, C, scale=0.2)
    gy = _rand(4, B, C, 1, P, positive=positive)
    _spike(gy, 3, [0, -1, 8191, 8192, 16383, 16384, 63, 64])       # ends of the row, of the apply chunks, of a stats tile
    _spike_cross(gy, 1, [0, -1, C1 - 1, C1], 3, [5, -7])           # ends of the sums over channels (m1, m2), at two pixels
    if B > 64:                                                     # ends of the finish chunks (64 samples each), at two pixels
        _spike_cross(gy, 0, [0, -1, 63, 64, 127, 128], 3, [2, -3])
    ct = _rand(5, B, C1, 1, P) if add else None
    J = _Judge(record_property, f"norm bwd B{B} C{C1}+{C2} P{P} add{int(add)} cond{int(badly_conditioned)}")

    def run(fn32, leaves):
        xs = leaves[0] if C2 == 0 else torch.cat(leaves[:2], 1)
        return fn32(xs, leaves[2], leaves[3])

    runs = []
    for _ in range(2):
        lv = [x1.clone().requires_grad_(True), x2.clone().requires_grad_(True) if C2 else None,
              w.clone().requires_grad_(True), b.clone().requires_grad_(True)]
        if add:      # the residual branch's gradient enters the apply kernel as addend1
            y, skip = ops.channel_norm_skip(lv[0], lv[2], lv[3], 1e-5, lv[1])
            torch.autograd.backward([y, skip], [gy, ct])
        else:
            y = ops.channel_norm(lv[0], lv[2], lv[3], 1e-5, lv[1])
            y.backward(gy)
        runs.append([y.detach()] + [t.grad for t in lv if t is not None])
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)                      # documented atomic-free (fixed-order partial sums)
    outs = []
    for leaf, fn in ((_leaf64, R.channel_norm), (_leaf32, O.channel_norm)):
        lv = [leaf(x1), leaf(x2) if C2 else None, leaf(w), leaf(b)]
        y = run(fn, lv)
        g, c_ = (gy.double(), ct.double() if add else None) if leaf is _leaf64 else (gy.cpu(), ct.cpu() if add else None)
        tot = (y * g).sum() + ((lv[0] * c_).sum() if add else 0.0)
        tot.backward()
        outs.append([y.detach()] + [t.grad for t in lv if t is not None])
    # sequential yardsticks of gw (terms gy xhat) and gb (terms gy) over the B P pixels, from fp32 CPU terms
    xc, gc = x.cpu(), gy.cpu()
    mean = xc.mean(1, keepdim=True)
    xhat = (xc - mean) * (((xc - mean) ** 2).sum(1, keepdim=True) / (C - 1) + 1e-5) ** -0.5
    seq_gw = _seq_sum((gc * xhat).permute(1, 0, 2, 3).reshape(C, -1))
    seq_gb = _seq_sum(gc.permute(1, 0, 2, 3).reshape(C, -1))
    names = ["y", "gx1"] + (["gx2"] if C2 else []) + ["gw", "gb"]
    for n, got, r, c_ in zip(names, runs[0], outs[0], outs[1]):
        J.add(n, got, r, c_, FWD if n == "y" else BWD, {"gw": seq_gw, "gb": seq_gb}.get(n))
    J.done()


# (B, C1, C2, P, addend): three apply chunks' worth of partial rows; the reaction block's concat, scalar path; two finish chunks
NORM_WS_CASES = [(3, 20, 0, 8196, False), (1, 1024, 128, 8191, True), (65, 20, 0, 100, False)]


@pytest.mark.parametrize("B,C1,C2,P,add", NORM_WS_CASES)
def test_channel_norm_backward_workspace(ops, L, B, C1, C2, P, add):
    """paradis_channel_norm_bwd_ws_bytes is what norm_bwd_plan lays out and no more: a call through the C ABI on a workspace
    of exactly that size leaves the 4096 canary bytes behind it alone, and returns the bytes of the op (which sizes its own
    workspace from the same query)."""
    C = C1 + C2
    x = _rand(1, B, C, 1, P, scale=3.0) + 1.0
    x1, x2 = x[:, :C1].contiguous(), (x[:, C1:].contiguous() if C2 else None)
    w, b = 1.0 + _rand(2, C, scale=0.2), _rand(3, C, scale=0.2)
    gy = _rand(4, B, C, 1, P)
    ct = _rand(5, B, C1, 1, P) if add else None
    _, mean, rstd = ops._channel_norm(x1, x2, w, b, 1e-5)
    want = ops._channel_norm_backward(gy, x1, x2, w, mean, rstd, ct)
    nbytes = L.lib.paradis_channel_norm_bwd_ws_bytes(B, C, P)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    got = [torch.full_like(t, -7.0) for t in want]
    rc = L.lib.paradis_channel_norm_bwd(L.dptr(gy), L.dptr(x1), L.dptr(x2), L.dptr(w), L.dptr(mean), L.dptr(rstd),
                                        L.dptr(got[0]), L.dptr(got[1]) if C2 else None, L.dptr(got[2]), L.dptr(got[3]), B, C1, C2,
                                        P, C1 * P, C2 * P, C1 * P, C2 * P, L.dptr(ct), C1 * P, L.dptr(ws), L.stream_ptr())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    assert not bool((ws[:nbytes - 256] == 0xA5).all())            # (the call did use the workspace handed in)
    for name, g, r in zip(("gx1", "gx2", "gw", "gb"), got, want):
        assert torch.equal(g, r), name


# ================================================================================================ element-wise
# elementwise.hip / train.hip: float4 path iff n % 4 == 0 and every pointer is 16-byte aligned; stream_blocks caps the grid at
# 4096 workgroups of 256 (one sweep = 4 * 4096 * 256 elements of the float4 path), blocks_for at 2048
SWEEP = 4 * 4096 * 256
EW_N = [1, 3, 4, 1023,
        SWEEP + 4,      # float4 path, one float4 into the second grid sweep
        SWEEP + 5]      # scalar path (n % 4 == 1), four sweeps and a tail


def _placed(vals, off):
    """vals in a view that starts `off` elements past a 16-byte boundary; the rest of the allocation holds a canary"""
    buf = torch.full((vals.numel() + 8,), -7.0, device="cuda")
    v = buf[off:off + vals.numel()]
    v.copy_(vals.reshape(-1))
    return buf, v


def _canary_ok(buf, off, n):
    return bool((buf[:off] == -7.0).all()) and bool((buf[off + n:] == -7.0).all())


def _act_values(n, act):
    """normal values with, in front, both tails on a log scale: |z| up to 90 (SiLU: exp(-z) overflows fp32 at 88.7) or
    6 (GELU: erf saturates) and values next to zero"""
    x = _rand(n, n, scale=3.0)
    top = 90.0 if act == 1 else 6.0
    tails = torch.logspace(-6, float(np.log10(top)), 64, device="cuda")
    tails = torch.cat([tails, -tails, torch.zeros(1, device="cuda")])[:n]
    x[:tails.numel()] = tails
    return x


@pytest.mark.parametrize("n", EW_N)
@pytest.mark.parametrize("act", [1, 2])
def test_activation(L, record_property, n, act):
    x, gy = _act_values(n, act), _rand(n + 1, n, positive=(n % 2 == 1))
    J = _Judge(record_property, f"act{act} n{n}")
    res = {}
    for off in (0, 1):                                 # aligned base (float4 path when n % 4 == 0) and base + 1 element
        (_, xv), (_, gv) = _placed(x, off), _placed(gy, off)
        ybuf, yv = _placed(torch.zeros(n, device="cuda"), off)
        gbuf, gxv = _placed(torch.zeros(n, device="cuda"), off)
        ybuf.fill_(-7.0), gbuf.fill_(-7.0)
        assert L.lib.paradis_act_fwd(L.dptr(xv), L.dptr(yv), n, act, L.stream_ptr()) == 0, L.last_error()
        assert L.lib.paradis_act_bwd(L.dptr(gv), L.dptr(xv), L.dptr(gxv), n, act, L.stream_ptr()) == 0, L.last_error()
        assert _canary_ok(ybuf, off, n) and _canary_ok(gbuf, off, n)
        res[off] = (yv.clone(), gxv.clone())
    # same per-element arithmetic on both paths: the same bits
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    xr, xc = _leaf64(x), _leaf32(x)
    yr = R.act(xr, act)
    yc = F.silu(xc) if act == 1 else F.gelu(xc)
    yr.backward(gy.double())
    yc.backward(gy.cpu())
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
    J.add("y", res[0][0], yr, yc, FWD)
    J.add("gx", res[0][1], xr.grad, xc.grad, BWD)
    core = x.abs() <= 4.0                              # without the tails, whose magnitude would set the scale alone
    if bool(core.any()):
        J.add("y (|z| <= 4)", res[0][0][core], yr.detach()[core], yc.detach()[core.cpu()], FWD)
        J.add("gx (|z| <= 4)", res[0][1][core], xr.grad[core], xc.grad[core.cpu()], BWD)
    J.done()


@pytest.mark.parametrize("n", EW_N)
def test_add_scale_copy(L, n):
    """paradis_add / _add_bcast / _scale / _copy_channels: one correctly rounded operation per element, so the result is
    the fp64 result rounded once - bit for bit, on the float4 and the scalar path, with nothing written past the end"""
    a, b = _rand(1, n), _rand(2, n, positive=True)
    k = torch.tensor([0.37], device="cuda")
    want_add = (a.double() + b.double()).float()
    want_scale = (a.double() * k.double()).float()
    for off in (0, 1):
        (_, av), (_, bv) = _placed(a, off), _placed(b, off)
        ybuf, yv = _placed(torch.zeros(n, device="cuda"), off)
        ybuf.fill_(-7.0)
        assert L.lib.paradis_add(L.dptr(av), L.dptr(bv), L.dptr(yv), n, L.stream_ptr()) == 0, L.last_error()
        assert torch.equal(yv, want_add) and _canary_ok(ybuf, off, n)
        ybuf.fill_(-7.0)
        assert L.lib.paradis_scale(L.dptr(av), L.dptr(k), L.dptr(yv), n, L.stream_ptr()) == 0, L.last_error()
        assert torch.equal(yv, want_scale) and _canary_ok(ybuf, off, n)
    # broadcast add over B = 3 samples of n elements; channel-block copy between different batch strides
    B = 3
    x = _rand(3, B, n)
    for off in (0, 1):
        (_, xv), (_, mv) = _placed(x, off), _placed(b, off)
        ybuf, yv = _placed(torch.zeros(B * n, device="cuda"), off)
        ybuf.fill_(-7.0)
        assert L.lib.paradis_add_bcast(L.dptr(xv), L.dptr(mv), L.dptr(yv), n, B, L.stream_ptr()) == 0, L.last_error()
        assert torch.equal(yv.view(B, n), (x.double() + b.double()).float()) and _canary_ok(ybuf, off, B * n)
    src = _rand(4, B, n + 3)
    dst = torch.full((B, n + 5), -7.0, device="cuda")
    assert L.lib.paradis_copy_channels(L.dptr(src), n + 3, L.dptr(dst), n + 5, B, n, L.stream_ptr()) == 0, L.last_error()
    assert torch.equal(dst[:, :n], src[:, :n]) and bool((dst[:, n:] == -7.0).all())


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (97, 1030)])    # 32x32 tiles: one partial, ragged both ways, exact, many + ragged
def test_transpose(L, rows, cols):
    x = _rand(1, rows, cols)
    buf, out = _placed(torch.zeros(rows * cols, device="cuda"), 0)
    buf.fill_(-7.0)
    assert L.lib.paradis_transpose(L.dptr(x), L.dptr(out), rows, cols, L.stream_ptr()) == 0, L.last_error()
    assert torch.equal(out.view(cols, rows), x.t().contiguous()) and _canary_ok(buf, 0, rows * cols)


# ================================================================================================ gated blend
@pytest.mark.parametrize("B,C,P", [(2, 5, 128),            # the tiny shape; strictly positive terms
                                   (3, 7, 130),            # P not a multiple of the 256-thread stride or of 4
                                   (32, 1024, 2048)])      # production B C P: galpha sums 65 536 terms per channel
def test_gated_blend(ops, record_property, B, C, P):
    positive = (B, C, P) == (2, 5, 128)
    h, alpha = _rand(1, B, C, 1, P), _rand(2, C)
    adv = h + _rand(3, B, C, 1, P, positive=True) if positive else _rand(3, B, C, 1, P)
    gout = _rand(4, B, C, 1, P, positive=positive)
    _spike(gout, 3, [0, -1, 255, 256, P - 2])
    _spike_cross(gout, 0, [0, -1], 3, [5, -7])                    # ends of the sum over the batch (gated_blend_finish)
    J = _Judge(record_property, f"blend {B}x{C}x{P}")
    out = ops._gated_blend(h, adv, alpha)
    r1 = ops._gated_blend_backward(gout, h, adv, alpha)
    r2 = ops._gated_blend_backward(gout, h, adv, alpha)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)                       # per-plane partials, summed over b in order: no atomics
    ro = ops._gated_blend_backward_out(gout, h, out, alpha)
    lr, lc = [_leaf64(t) for t in (h, adv, alpha)], [_leaf32(t) for t in (h, adv, alpha)]
    yr = R.gated_blend(*lr)
    yc = lc[0] + torch.sigmoid(lc[2]).view(1, -1, 1, 1) * (lc[1] - lc[0])
    yr.backward(gout.double())
    yc.backward(gout.cpu())
    gc = torch.sigmoid(alpha.cpu())
    seq = _seq_sum((gout.cpu() * (adv.cpu() - h.cpu())).permute(1, 0, 2, 3).reshape(C, -1)) * gc * (1 - gc)
    J.add("out", out, yr, yc, FWD)
    for tag, res in (("", r1), (" (from out)", ro)):   # both entry points are defined algebraically: both against fp64
        J.add("gh" + tag, res[0], lr[0].grad, lc[0].grad, BWD)
        J.add("gadv" + tag, res[1], lr[1].grad, lc[1].grad, BWD)
        J.add("galpha" + tag, res[2], lr[2].grad, lc[2].grad, BWD, seq)
    J.done()


# ================================================================================================ bias grads
# elementwise.hip: bias_grads_vec4_kernel iff P % 4 == 0, dz_bs % 4 == 0 and 16-byte aligned dz / gmap, else bias_grads_kernel;
# pchunks = min(2, ceil(P4 / 256), 2048 / C) workgroups per channel, their two atomic adds into gbias commute
BG_CASES = [
    # (B, C, P, channel slice of a wider tensor, elements past a 16-byte boundary)
    (1, 5, 128, False, 0), (7, 5, 128, False, 0),      # B < 8: only the tail of the batch unroll
    (8, 5, 128, False, 0), (9, 5, 128, False, 0),      # one full batch of 8; one batch + 1
    (7, 5, 128, False, 1),                             # same values, misaligned base: the scalar kernel
    (9, 5, 130, False, 0),                             # P % 4 != 0: the scalar kernel
    (8, 6, 2048, True, 0),                             # dz_bs != C P (a channel slice); pchunks = 2
    (9, 2, 4100, False, 0),                            # P4 = 1025: a thread's second column, pchunks = 2
    (9, 2, 4102, True, 0),                             # the scalar kernel with pchunks = 2 on a slice
    (9, 1025, 2048, False, 0),                         # 2048 / C = 1: pchunks = 1
    (32, 1024, 2048, False, 0),                        # production: pchunks = 2
]


def _bg_inputs(B, C, P, sliced, off, positive):
    vals = _rand(1, B, C, P, positive=positive)
    _spike(vals, 2, [0, -1, 1023, 1024, 2047, 255, 256])           # ends of the row and of the 256-column strides
    _spike_cross(vals, 0, [0, -1, 7, 8], 2, [5, -7, 1030])         # ends of the batch sum and of its unroll by 8
    Cw = C + 3 if sliced else C
    buf = torch.full((B * Cw * P + 8,), -7.0, device="cuda")
    wide = buf[off:off + B * Cw * P].view(B, Cw, P)
    dz = wide[:, 2:2 + C] if sliced else wide
    dz.copy_(vals)
    return vals, dz, Cw * P


def _bg_call(L, dz, bs, B, C, P):
    gmap, gb = torch.full((C, P), -7.0, device="cuda"), torch.full((C,), -7.0, device="cuda")
    rc = L.lib.paradis_bias_grads(L.dptr(dz), L.dptr(gmap), L.dptr(gb), B, C, P, bs, L.stream_ptr())
    assert rc == 0, L.last_error()
    return gmap, gb


@pytest.mark.parametrize("B,C,P,sliced,off", BG_CASES)
def test_bias_grads(L, record_property, B, C, P, sliced, off):
    vals, dz, bs = _bg_inputs(B, C, P, sliced, off, positive=(B % 2 == 1))
    assert (dz.data_ptr() % 16 == 0) == (off == 0 and (not sliced or (2 * P) % 4 == 0))
    J = _Judge(record_property, f"bias_grads {B}x{C}x{P} slice{int(sliced)} off{off}")
    gmap, gb = _bg_call(L, dz, bs, B, C, P)
    gmap2, gb2 = _bg_call(L, dz, bs, B, C, P)
    assert torch.equal(gmap, gmap2) and torch.equal(gb, gb2)      # pchunks <= 2: the header's claim that two adds commute
    rmap, rb = R.bias_grads(vals.double())
    vc = vals.cpu()
    J.add("gmap", gmap, rmap, vc.sum(0), BWD)
    J.add("gbias", gb, rb, vc.sum((0, 2)), BWD, _seq_sum(vc.permute(1, 0, 2).reshape(C, -1)))
    # only one of the two outputs asked for
    only = torch.full((C,), -7.0, device="cuda")
    assert L.lib.paradis_bias_grads(L.dptr(dz), None, L.dptr(only), B, C, P, bs, L.stream_ptr()) == 0
    assert torch.equal(only, gb)
    J.done()


_DET_CHILD = r"""
import json, sys, torch
sys.path.insert(0, %r)
from tests import test_hip_kernel_edges as T
from paradis_model_amd import _lib as L
out = {}
for B, C, P, sliced, off in ((9, 6, 2048, False, 0), (9, 2, 4102, True, 0)):
    vals, dz, bs = T._bg_inputs(B, C, P, sliced, off, True)
    a, b = T._bg_call(L, dz, bs, B, C, P), T._bg_call(L, dz, bs, B, C, P)
    rmap, rb = T.R.bias_grads(vals.double())
    out[str(P)] = dict(equal=bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])), e_map=T._e(a[0], rmap), e_b=T._e(a[1], rb),
                       e_cpu=max(T._e(vals.cpu().sum((0, 2)), rb), T._e(T._seq_sum(vals.cpu().permute(1, 0, 2).reshape(C, -1)), rb)))
print("RESULT " + json.dumps(out))
"""


def test_bias_grads_deterministic_mode(record_property):
    """PARADIS_DETERMINISTIC=1 (read when the library is first used, hence the child process): one workgroup per
    channel, no atomics; two runs bit-identical, same bounds against fp64"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PARADIS_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", _DET_CHILD % root], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for key, v in res.items():
        print(f"EDGE | bias_grads deterministic P{key} | gbias | e_hip {v['e_b']:.2e} | e_cpu {v['e_cpu']:.2e}")
        record_property(key, json.dumps(v))
        assert v["equal"]
        assert v["e_map"] <= BWD and v["e_b"] <= BWD and v["e_b"] <= 1.5 * v["e_cpu"] + 1e-7, v


# ================================================================================================ loss
# train.hip: blocks_for caps the grid at 2048 workgroups of 256: one sweep = 2048 * 256 elements; 2048 partials, summed
# in double by loss_finish_kernel
LOSS_SWEEP = 2048 * 256


@pytest.mark.parametrize("kind", ["mse", "reversed_huber"])
@pytest.mark.parametrize("with_wl", [True, False])                   # wl == NULL
@pytest.mark.parametrize("delta", [0.25, 1.0, 3.0])
@pytest.mark.parametrize("shape", [(2, 97, 32, 64),                  # < one sweep: 1552 workgroups
                                   (1, 3, 5, 7),                     # one partly filled workgroup
                                   (2, 17, 256, 256)])               # total = 2 228 224 > 2048 * 256 * 4: five sweeps, ragged last
def test_loss(ops, record_property, kind, with_wl, delta, shape):
    B, C, H, W = shape
    total = B * C * H * W
    target = _rand(1, *shape)
    g = torch.Generator(device="cuda").manual_seed(2)
    mag = 10.0 ** (torch.rand(*shape, generator=g, device="cuda") * 6.0 - 4.0)         # |e| log-uniform over [1e-4, 1e2]
    sign = torch.where(torch.rand(*shape, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    pred = target + sign * mag
    pf, tf = pred.view(-1), target.view(-1)
    z0, z1 = min(40, total // 3), min(40, total // 3) + min(64, total // 3)
    pf[z0:z1] = tf[z0:z1]                                            # a block with pred == target exactly (dl = 0 branch)
    for i in (0, total - 1, LOSS_SWEEP - 1, LOSS_SWEEP, 4 * LOSS_SWEEP - 1, 4 * LOSS_SWEEP):
        if i < total:                                                # first / last element, both sides of a sweep boundary:
            pf[i] = tf[i] + 100.0                                    # the largest |e| of the range
    wf = _rand(3, C, positive=True)
    wl = _rand(4, H, positive=True) if with_wl else None
    J = _Judge(record_property, f"loss {kind} wl{int(with_wl)} delta{delta} {B}x{C}x{H}x{W}")
    grads = []
    for scale in (None, 0.37):                                       # the gradient, and under an upstream scale
        p = pred.clone().requires_grad_(True)
        val = ops.paradis_loss(p, target, wf, wl, kind, delta)
        (val if scale is None else val * scale).backward()
        grads.append(p.grad)
    assert bool((grads[0].view(-1)[z0:z1] == 0).all())
    code = {"mse": 0, "reversed_huber": 1}[kind]
    pr, pc = _leaf64(pred), _leaf32(pred)
    vr = R.loss(pr, target.double(), wf.double(), wl.double() if with_wl else None, code, delta)
    vc = O.paradis_loss(pc, target.cpu(), wf.cpu(), wl.cpu() if with_wl else None, kind, delta)
    vr.backward()
    vc.backward()
    # the value: a sum over `total` terms; sequential yardstick over the oracle's fp32 per-element terms
    with torch.no_grad():
        lt = O.reversed_huber(pred.cpu(), target.cpu(), delta) if code else (pred.cpu() - target.cpu()) ** 2
        lt = lt * wf.cpu().view(1, -1, 1, 1)
        if with_wl:
            lt = lt * wl.cpu().view(1, 1, -1, 1)
        seq = _seq_sum(lt.reshape(1, -1)) / np.float32(total)
    J.add("value", val.detach().view(1), vr.detach().view(1), vc.detach().view(1), FWD, seq if total >= 256 else None)
    J.add("grad", grads[0], pr.grad, pc.grad, BWD)
    J.add("grad x 0.37", grads[1], pr.grad * 0.37, pc.grad * np.float32(0.37), BWD)
    J.done()


# ================================================================================================ AdamW
# train.hip: adamw_multi_kernel, one workgroup per chunk of ADAMW_CHUNK = 32768 elements of one tensor
@pytest.mark.parametrize("mode", ["multi",           # one launch for the group, bias corrections from the host
                                  "capturable",      # the dev_state branch: step count and lr read on the device
                                  "single"])         # one-tensor groups: adamw_kernel, grid-stride
def test_adamw(record_property, mode):
    """Finding of this test: with 1 - beta formed in fp32 from the fp32-rounded betas (1.0f - 0.9f = 0.10000002) m and v
    were 2.5e-7 ... 3.0e-7 off against torch's 4e-8 ... 8e-8 - inside the 1e-6 ceiling, outside the fp32 yardstick.  The
    coefficients are now formed in double (paradis_adamw_*_d): m and v carry torch's own error."""
    from paradis_model_amd._lib import lib
    from paradis_model_amd.optim import AdamW
    assert lib.paradis_adamw_chunk() == 32768
    sizes = [32768,      # exactly one chunk
             32769,      # one chunk and a one-element chunk
             65536,      # two full chunks
             1]
    kw = dict(lr=5e-4, weight_decay=1e-2, betas=(0.9, 0.95), eps=1e-8)
    # (element-wise: every element carries the same weight in the metric, the chunk edges included; no spikes)
    ps = [_rand(10 + i, n) for i, n in enumerate(sizes)]
    gs = [[_rand(100 * s + i, n, scale=10.0 ** (s - 1)) for i, n in enumerate(sizes)] for s in range(3)]
    mine = [torch.nn.Parameter(p.clone()) for p in ps]
    cpu = [torch.nn.Parameter(p.cpu().clone()) for p in ps]
    if mode == "single":
        o_mine = AdamW([dict(params=[p]) for p in mine], **kw)
    else:
        o_mine = AdamW(mine, capturable=(mode == "capturable"), **kw)
    o_cpu = torch.optim.AdamW(cpu, **kw)
    ref = [(p.double(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)) for p in ps]
    for s in range(3):
        for m, c, g in zip(mine, cpu, gs[s]):
            m.grad, c.grad = g.clone(), g.cpu().clone()
        o_mine.step()
        o_cpu.step()
        ref = [R.adamw_step(p, g.double(), m, v, s + 1, kw["lr"], 0.9, 0.95, kw["eps"], kw["weight_decay"])
               for (p, m, v), g in zip(ref, gs[s])]
    J = _Judge(record_property, f"adamw {mode}")
    for i, (m, c, (p, m1, v1)) in enumerate(zip(mine, cpu, ref)):
        sm, sc = o_mine.state[m], o_cpu.state[c]
        J.add(f"p[{sizes[i]}]", m, p, c, ADAM)
        J.add(f"m[{sizes[i]}]", sm["exp_avg"], m1, sc["exp_avg"], ADAM)
        J.add(f"v[{sizes[i]}]", sm["exp_avg_sq"], v1, sc["exp_avg_sq"], ADAM)
    J.done()


# ---- the pointwise GEMMs' weight gradient, once per kernel of its plan --------------------------------------------------
# (scheme, dz stored as bf16, x stored as bf16, B, Co, Ci, H, W, x is a channel slice of a wider tensor); each shape is the
# smallest that reaches its kernel by the predicates of wgrad_kind (csrc/gemm_common.h) - tools/gemm_plan_check.hip prints
# the kernel it picks for every one of them and fails unless all seven occur
_WGRAD_KINDS = {
    "register-staged (P % 16 != 0)":     ("exact", False, False, 2, 5, 3, 6, 10, False),
    "f32 DMA":                           ("exact", False, False, 2, 5, 3, 8, 8, False),
    "f32 DMA, one slab":                 ("exact", False, False, 1, 5, 3, 4, 4, False),
    "f32 DMA, sliced x":                 ("exact", False, False, 2, 5, 3, 8, 8, True),
    "bf16x3 split":                      ("bf16x3", False, False, 2, 5, 3, 8, 8, False),
    "bf16x3 split, one slab":            ("bf16x3", False, False, 1, 5, 3, 4, 4, False),
    "bf16x3 split, sliced x":            ("bf16x3", False, False, 2, 5, 3, 8, 8, True),
    "f16x2 split":                       ("f16x2", False, False, 2, 5, 3, 8, 8, False),
    "f16x2 split, one slab":             ("f16x2", False, False, 1, 5, 3, 4, 4, False),
    "bf16-mixed 128x128, fp32 operands": ("bf16", False, False, 2, 5, 3, 8, 8, False),
    "bf16-mixed 128x128, bf16 dz":       ("bf16", True, False, 2, 5, 3, 8, 8, False),
    "bf16-mixed 128x128, bf16 x":        ("bf16", False, True, 2, 5, 3, 8, 8, False),
    "bf16-mixed 128x128, both bf16":     ("bf16", True, True, 2, 5, 3, 8, 8, False),
    "tall":                              ("bf16", False, False, 2, 256, 8, 4, 8, False),
    "tall, ragged second tile":          ("bf16", False, False, 2, 448, 8, 4, 8, False),
    "tall, sliced bf16 x":               ("bf16", False, True, 2, 256, 8, 4, 8, True),
    "square":                            ("bf16", False, False, 2, 256, 224, 4, 8, False),
}


@pytest.mark.parametrize("kind", list(_WGRAD_KINDS))
def test_wgrad_every_kind_exact(ops, kind):
    """dW = sum_b dz x^T and the bias gradient (row sums of dz) through ops.RAW["pw_gemm_wgrad"], once per kernel the
    plan can choose.  Operands are integers in [-4, 4]: exact as bf16, every product and every partial sum an integer of
    magnitude <= 16 B P < 2^24, so fp32 accumulation in any order, the slab sums and the f16x2 scheme's power-of-two
    scaling are all exact - the tolerance against fp64 is zero by construction, not by measurement (the method of
    test_split_exactness_on_bf16_representable_inputs)."""
    scheme, dz16, x16, B, Co, Ci, H, W, sliced = _WGRAD_KINDS[kind]
    assert 16 * B * H * W < 2 ** 24
    g = torch.Generator().manual_seed(Co * 1000 + Ci + H)
    dz = torch.randint(-4, 5, (B, Co, H, W), generator=g).float().cuda()
    wide = torch.randint(-4, 5, (B, Ci + 2, H, W), generator=g).float().cuda()
    if dz16:
        dz = dz.bfloat16()
    if x16:
        wide = wide.bfloat16()
    x = wide[:, 1:1 + Ci] if sliced else wide[:, 1:1 + Ci].contiguous()
    assert sliced == (B > 1 and x.stride(0) != Ci * H * W)
    code = {"exact": ops.GEMM_EXACT, "bf16": ops.GEMM_BF16, "f16x2": ops.GEMM_F16X2, "bf16x3": ops.GEMM_BF16X3}[scheme]
    gw, gb = ops.RAW["pw_gemm_wgrad"](dz, x, True, None, None, code)
    torch.cuda.synchronize()
    ref_w = torch.einsum("bmhw,bkhw->mk", dz.double(), x.double())
    ref_b = dz.double().sum(dim=(0, 2, 3))
    assert gw.dtype == torch.float32 and gw.shape == (Co, Ci) and gb.shape == (Co,)
    assert torch.equal(gw.double(), ref_w), (kind, float((gw.double() - ref_w).abs().max()))
    assert torch.equal(gb.double(), ref_b), (kind, float((gb.double() - ref_b).abs().max()))
