"""The sign copies of the six-product (bf16x3) GEMM k-loops, exactly.

Claim under test (csrc/gemm_split.hip ``pw_gemm_split_wide_kernel``, csrc/gemm_common.h ``pw_gemm_wgrad_split_kernel``):
a staging wave (forward / data gradient) or a workgroup (weight gradient) picks, once, the plain or the negated copy of
prologue and k-loop, the weight gradient also the copy with or without the fused row sums, and interior tiles of the weight
gradient leave through the straight-line store epilogue - and the result is what it always was.

Every input is integer valued with |value| <= 64 (smaller where a sum has more terms: the bound is chosen per case so
that terms x max |product| stays below 2^24), so every product and every partial sum is exact in fp32 in any order and
the GEMM must EQUAL the exact reference: a wrong sign, a dropped plane or a missed flip-back has no tolerance to hide
behind.  The reference is a float64 product on the device (exact: every sum is far below 2^53) taken to int64.

Forward / data gradient: M in {128, 256} x N in {128 (the 128 x 128 kernel), 256 (both column blocks of both halves),
384 (an idle second half), 200 (ragged)} x K in {16, 32, 48, 1040} (one, two, three k-tiles - prologue and surplus
split in both copies - and a long loop), without options and with bias + SiLU + saved pre-activation.
Weight gradient: M x K' in {128 x 128, 128 x 256, 256 x 128, 97 x 200}, B x P chosen from the plan's slab count S (>= 2:
odd and even slabs) so that a slab is 1, 1 or 2, 2, 3 and 9 k-tiles long, with and without the fused row sums.
The same launches under PARADIS_GEMM_EPILOGUE=generic (read at every launch) must give the same bits."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_M = [128, 256]
FWD_N = {128: (2, 64), 256: (4, 64), 384: (6, 64), 200: (5, 40)}      # N -> (H, W)
FWD_K = [16, 32, 48, 1040]
FWD_B = 2
WGRAD_MK = [(128, 128), (128, 256), (256, 128), (97, 200)]
WGRAD_LEN = [1.0, 1.5, 2.0, 3.0, 9.0]       # k-tiles per slab (1.5: slabs of one and of two tiles alternate)
WGRAD_B = 2


@pytest.fixture(scope="module")
def ops():
    from paradis_model_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def _generic_epilogue():
    keep = os.environ.get("PARADIS_GEMM_EPILOGUE")
    os.environ["PARADIS_GEMM_EPILOGUE"] = "generic"
    try:
        yield
    finally:
        if keep is None:
            del os.environ["PARADIS_GEMM_EPILOGUE"]
        else:
            os.environ["PARADIS_GEMM_EPILOGUE"] = keep


def _ints(seed, *shape, vmax=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-vmax, vmax + 1, shape, generator=g).float()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _exact(t):
    """an fp32 tensor of integers as int64 (asserting that it holds integers and nothing else)"""
    assert bool(torch.isfinite(t).all())
    i = t.to(torch.int64)
    assert torch.equal(i.float(), t), "not integer valued"
    return i


# ---- forward / data gradient --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd_inputs():
    """one activation tensor per (N, K) and one weight per (M, K), shared by all cases (nothing writes to them);
    K = 1040 terms of at most 64 x 64 stay below 2^24 (plus a bias of at most 64)"""
    assert 1040 * 64 * 64 + 64 < 2 ** 24
    x = {(n, k): _ints(1000 + 7 * n + k, FWD_B, k, *FWD_N[n]).cuda() for n in FWD_N for k in FWD_K}
    w = {(m, k): _ints(2000 + 3 * m + k, m, k, 1, 1).cuda() for m in FWD_M for k in FWD_K}
    b = {m: _ints(3000 + m, m).cuda() for m in FWD_M}
    # the data gradient reduces over M: dz [B, K (its reduction length), H, W] through the weight [K, M]
    wd = {(m, k): _ints(4000 + 3 * m + k, k, m, 1, 1).cuda() for m in FWD_M for k in FWD_K}
    return {"x": x, "w": w, "b": b, "wd": wd}


def _forward(ops, x, w, b, opts):
    from paradis_model_amd.ops._core import ACT_CODES
    from paradis_model_amd.ops.gemm import _pointwise
    y, z, _ = _pointwise(x=x, weight=w, bias=b if opts else None, bmap=None, residual=None,
                         act=ACT_CODES["SiLU" if opts else None], x_pre=None, x_act=0, defer_act_grad=False, m8=None, pw=None,
                         save_z=bool(opts), scheme=ops._SCHEMES["bf16x3"], gate=None)
    torch.cuda.synchronize()
    return y, z


@pytest.mark.parametrize("opts", [False, True], ids=["none", "bias+SiLU+z"])
@pytest.mark.parametrize("K", FWD_K)
@pytest.mark.parametrize("N", list(FWD_N))
@pytest.mark.parametrize("M", FWD_M)
def test_forward_is_exact(ops, fwd_inputs, M, N, K, opts):
    x, w, b = fwd_inputs["x"][(N, K)], fwd_inputs["w"][(M, K)], fwd_inputs["b"][M]
    y, z = _forward(ops, x, w, b, opts)
    ref = torch.einsum("mk,bkn->bmn", w.reshape(M, K).double(), x.reshape(FWD_B, K, N).double())
    if opts:
        ref = ref + b.double()[None, :, None]
    ref = ref.to(torch.int64).reshape(FWD_B, M, *FWD_N[N])
    pre = z if opts else y
    bad = _exact(pre) != ref
    assert not bool(bad.any()), "%d of %d elements differ from the exact product" % (int(bad.sum()), bad.numel())
    # (y = SiLU(z) is no integer: it is held to the generic epilogue's bits below, and that to its reference elsewhere)
    with _generic_epilogue():
        y_g, z_g = _forward(ops, x, w, b, opts)
    assert _same_bits(y, y_g) and _same_bits(z, z_g), "the compiled-in and the generic epilogue differ"


@pytest.mark.parametrize("K", FWD_K)
@pytest.mark.parametrize("N", list(FWD_N))
@pytest.mark.parametrize("M", FWD_M)
def test_data_gradient_is_exact(ops, fwd_inputs, M, N, K):
    from paradis_model_amd.ops.gemm import _pw_gemm_dgrad
    dz, wd = fwd_inputs["x"][(N, K)], fwd_inputs["wd"][(M, K)]

    def run():
        dx = _pw_gemm_dgrad(dz=dz, weight=wd, zmul=None, x_act=0, dz_amax=None, scheme=ops._SCHEMES["bf16x3"])
        torch.cuda.synchronize()
        return dx

    dx = run()
    ref = torch.einsum("km,bkn->bmn", wd.reshape(K, M).double(), dz.reshape(FWD_B, K, N).double()).to(torch.int64)
    bad = _exact(dx).reshape(FWD_B, M, N) != ref
    assert not bool(bad.any()), "%d of %d elements differ from the exact product" % (int(bad.sum()), bad.numel())
    with _generic_epilogue():
        assert _same_bits(dx, run()), "the compiled-in and the generic epilogue differ"


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
def _wgrad_case(M, Kp, length):
    """(P, S, vmax): P points per sample so that the plan's S slabs are `length` k-tiles (of 16 points) long on average"""
    from paradis_model_amd._lib import lib
    s_max = lib.paradis_pw_gemm_wgrad_slabs(WGRAD_B, M, Kp, 1 << 24)      # the slab count of a long reduction
    P = int(16 * length * s_max) // WGRAD_B
    S = lib.paradis_pw_gemm_wgrad_slabs(WGRAD_B, M, Kp, P)
    terms = WGRAD_B * P
    vmax = 64
    while terms * vmax * vmax >= 2 ** 24:      # every partial sum of products (and of values: the row sums) exact in fp32
        vmax -= 1
    return P, S, vmax


@pytest.fixture(scope="module")
def wgrad_inputs():
    """operands and exact references per (shape, slab length), computed once"""
    out = {}
    for i, (M, Kp) in enumerate(WGRAD_MK):
        for j, length in enumerate(WGRAD_LEN):
            P, S, vmax = _wgrad_case(M, Kp, length)
            dz = _ints(5000 + 10 * i + j, WGRAD_B, M, 1, P, vmax=vmax).cuda()
            x = _ints(6000 + 10 * i + j, WGRAD_B, Kp, 1, P, vmax=vmax).cuda()
            gw = torch.einsum("bmp,bkp->mk", dz.reshape(WGRAD_B, M, P).double(), x.reshape(WGRAD_B, Kp, P).double())
            gb = dz.double().sum(dim=(0, 2, 3))
            out[(M, Kp, length)] = {"dz": dz, "x": x, "gw": gw.to(torch.int64), "gb": gb.to(torch.int64), "P": P, "S": S,
                                    "vmax": vmax}
    return out


@pytest.mark.parametrize("want_bias", [False, True], ids=["no row sums", "row sums"])
@pytest.mark.parametrize("length", WGRAD_LEN)
@pytest.mark.parametrize("M,Kp", WGRAD_MK)
def test_weight_gradient_is_exact(ops, wgrad_inputs, M, Kp, length, want_bias):
    from paradis_model_amd.ops.gemm import _pw_gemm_wgrad
    d = wgrad_inputs[(M, Kp, length)]
    total_kt = WGRAD_B * d["P"] // 16
    assert d["S"] >= 2 and d["S"] % 2 == 0 and d["P"] % 16 == 0 and d["vmax"] >= 8
    assert total_kt == int(length * d["S"]), "the slabs are not `length` k-tiles long"

    def run():
        gw, gb = _pw_gemm_wgrad(dz=d["dz"], x=d["x"], want_bias=want_bias, dz_amax=None, x_amax=None,
                                scheme=ops._SCHEMES["bf16x3"])
        torch.cuda.synchronize()
        return gw, gb

    gw, gb = run()
    bad = _exact(gw) != d["gw"]
    assert not bool(bad.any()), "dW: %d of %d elements differ from the exact product" % (int(bad.sum()), bad.numel())
    assert gb.numel() == (M if want_bias else 0)
    if want_bias:
        assert torch.equal(_exact(gb), d["gb"]), "the row sums differ from the exact sums"
    with _generic_epilogue():
        gw_g, gb_g = run()
    assert _same_bits(gw, gw_g) and _same_bits(gb, gb_g), "the store epilogue and the generic epilogue differ"
