"""The split pointwise GEMMs (fp32 in / fp32 accumulate / fp32 out on the bf16 / f16 matrix pipe) against
the exact f32-MFMA kernels and an fp64 evaluation of the same product.

Claim under test (include/paradis_hip.h, a6): the split paths are fp32 GEMMs, not reduced-precision ones:
their error against fp64 is not above the exact f32 chain's.  Bounds written here, for "bf16x3" (exact
three-term decomposition, the default) and for "f16x2" (two f16 terms of the per-tensor scaled operands, opt-in):
  * max |split - fp64| / max |fp64|  <=  1.25 x the same figure of the exact kernel + 1e-7, and
  * <= 2e-6 absolutely (an fp32 dot product of length <= 1024 with |x|,|w| ~ 1 sits at ~3e-7).
What f16x2 gives up - relative accuracy of elements far below their TENSOR's largest magnitude - and its
all-or-nothing treatment of non-finite operands have their own tests below."""
import pytest
import torch

from tests._util import seeded

pytestmark = pytest.mark.gpu

SHAPES = [  # B, Ci, Co, H, W
    (2, 10, 7, 12, 16),        # one ragged tile, K < 16
    (2, 186, 64, 16, 32),      # K % 16 != 0 (the input projection's 186 channels)
    (3, 128, 97, 32, 64),      # M ragged
    (1, 256, 384, 17, 32),     # N = 544: ragged n tile, still N % 16 == 0
    (2, 130, 258, 9, 20),      # N = 180: weight-gradient falls back to the exact kernel (N % 16 != 0)
    (2, 1024, 896, 32, 64),    # the default model's widest GEMM
]


@pytest.fixture(scope="module")
def ops():
    from paradis_model_amd import ops as _ops
    return _ops


SPLIT_SCHEMES = ["f16x2", "bf16x3"]


def _run(ops, scheme, x, w, b, res, ct, act):
    keep = ops.GEMM_SCHEME
    ops.GEMM_SCHEME = ops._SCHEMES[scheme]
    try:
        ds = [t.detach().clone().cuda().requires_grad_(True) for t in (x, w, b, res)]
        y = ops.pointwise(ds[0], ds[1], ds[2], None, ds[3], act)
        y.backward(ct.cuda())
        torch.cuda.synchronize()
        return [y.detach()] + [d.grad for d in ds[:3]]
    finally:
        ops.GEMM_SCHEME = keep


def _fp64(x, w, b, res, ct, act):
    ts = [t.detach().clone().cuda().double().requires_grad_(True) for t in (x, w, b, res)]
    z = torch.einsum("oc,bchw->bohw", ts[1], ts[0]) + ts[2].view(1, -1, 1, 1)
    if act == "SiLU":
        z = torch.nn.functional.silu(z)
    elif act == "GELU":
        z = torch.nn.functional.gelu(z)
    y = z + ts[3]
    y.backward(ct.cuda().double())
    return [y.detach()] + [t.grad for t in ts[:3]]


def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("B,Ci,Co,H,W", SHAPES)
@pytest.mark.parametrize("act", [None, "SiLU"])
@pytest.mark.parametrize("scheme", SPLIT_SCHEMES)
def test_split_not_less_accurate_than_exact_f32(ops, scheme, B, Ci, Co, H, W, act):
    x = seeded(1, B, Ci, H, W)
    w = seeded(2, Co, Ci, scale=Ci ** -0.5)
    b = seeded(3, Co, scale=0.1)
    res = seeded(5, B, Co, H, W)
    ct = seeded(6, B, Co, H, W)
    ref = _fp64(x, w, b, res, ct, act)
    exact = _run(ops, "exact", x, w, b, res, ct, act)
    split = _run(ops, scheme, x, w, b, res, ct, act)
    for name, s, e, r in zip(("y", "gx", "gw", "gb"), split, exact, ref):
        es, ee = _err(s, r), _err(e, r)
        assert es <= 1.25 * ee + 1e-7, (name, es, ee)
        assert es <= 2e-6, (name, es)


def test_split_exactness_on_bf16_representable_inputs(ops):
    """Inputs that are exactly bf16 numbers with small integer values make every partial product and
    every partial sum exact in fp32 (f16x2: the power-of-two scaling is exact too): all three paths must
    then agree bit for bit with integer arithmetic."""
    g = torch.Generator().manual_seed(7)
    B, Ci, Co, H, W = 2, 64, 48, 8, 16
    x = torch.randint(-8, 9, (B, Ci, H, W), generator=g).float()
    w = torch.randint(-8, 9, (Co, Ci), generator=g).float()
    b = torch.zeros(Co)
    res = torch.zeros(B, Co, H, W)
    ct = torch.randint(-4, 5, (B, Co, H, W), generator=g).float()
    ref = _fp64(x, w, b, res, ct, None)
    for mode in ("f16x2", "bf16x3", "exact"):
        got = _run(ops, mode, x, w, b, res, ct, None)
        for name, a, r in zip(("y", "gx", "gw"), got, ref):
            assert torch.equal(a.double(), r), (mode, name)


def test_split_handles_wide_dynamic_range(ops):
    """bf16x3, operands spanning 12 decades: the h/m/l terms keep fp32's exponent range (bf16 has the same
    8 exponent bits), so nothing under- or overflows in the split."""
    g = torch.Generator().manual_seed(11)
    B, Ci, Co, H, W = 1, 96, 64, 8, 16
    mag = 10.0 ** (torch.rand(B, Ci, H, W, generator=g) * 12 - 6)
    x = torch.randn(B, Ci, H, W, generator=g) * mag
    w = torch.randn(Co, Ci, generator=g) * 10.0 ** (torch.rand(Co, Ci, generator=g) * 6 - 3)
    b = torch.zeros(Co)
    res = torch.zeros(B, Co, H, W)
    ct = torch.randn(B, Co, H, W, generator=g)
    ref = _fp64(x, w, b, res, ct, None)
    exact = _run(ops, "exact", x, w, b, res, ct, None)
    split = _run(ops, "bf16x3", x, w, b, res, ct, None)
    for name, s, e, r in zip(("y", "gx", "gw"), split, exact, ref):
        # element-wise relative to the fp64 magnitude scale of each output row/column is too strict
        # for cancelling sums; compare the two paths on the same max-normalised figure
        es, ee = _err(s, r), _err(e, r)
        assert es <= 1.25 * ee + 1e-7, (name, es, ee)


def test_f16x2_error_model(ops):
    """What the two-term scheme promises (include/paradis_hip.h): every operand element is represented
    to 2^-22 of itself or 2^-39 of its tensor's largest magnitude, whichever is larger.
      * tensors of any overall magnitude (1e-30 .. 1e+30): fp32-level result (the scale is per tensor);
      * a tensor whose samples differ by 2^12 in magnitude: the small samples' outputs still carry
        <= 2e-6 relative error (2^12 x 2^12 below the maxima on both operands is inside the 2^39 window);
      * entries 2^30 below the tensor's maximum: their contribution is right to 2^-39 of the maximum, i.e.
        the ABSOLUTE error of the output stays at fp32 level although those entries alone are not."""
    g = torch.Generator().manual_seed(21)
    B, Ci, Co, H, W = 2, 96, 64, 8, 16
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, generator=g) * Ci ** -0.5
    z = torch.zeros
    for sx, sw in ((1e30, 1e-30), (1e-30, 1e30), (1e-20, 1e-10), (1e15, 1e15)):
        ref = _fp64(x * sx, w * sw, z(Co), z(B, Co, H, W), torch.randn(B, Co, H, W, generator=g), None)
        got = _run(ops, "f16x2", x * sx, w * sw, z(Co), z(B, Co, H, W), torch.randn(B, Co, H, W, generator=g), None)
        assert _err(got[0], ref[0]) <= 2e-6, (sx, sw, _err(got[0], ref[0]))
    xs = x.clone()
    xs[1] *= 2.0 ** -12                       # second sample 2^12 below the first
    ct = torch.randn(B, Co, H, W, generator=g)
    ref = _fp64(xs, w, z(Co), z(B, Co, H, W), ct, None)
    got = _run(ops, "f16x2", xs, w, z(Co), z(B, Co, H, W), ct, None)
    assert _err(got[0][1], ref[0][1]) <= 2e-6 and _err(got[0][0], ref[0][0]) <= 2e-6
    assert _err(got[1][1], ref[1][1]) <= 2e-6       # gx of the small sample
    xt = x.clone()
    xt[:, ::2] *= 2.0 ** -30                  # every other channel 2^30 below the rest
    ref = _fp64(xt, w, z(Co), z(B, Co, H, W), ct, None)
    got = _run(ops, "f16x2", xt, w, z(Co), z(B, Co, H, W), ct, None)
    assert _err(got[0], ref[0]) <= 2e-6 and _err(got[2], ref[2]) <= 2e-6


def test_f16x2_non_finite_operand_poisons_the_product(ops):
    """An Inf or NaN anywhere in an operand tensor makes its largest magnitude non-finite: the whole
    product comes out NaN (loudly wrong), never silently rescaled.  bf16x3 / exact confine it to the
    outputs it touches (test_split_extreme_magnitudes)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 8, 16, generator=g)
    w = torch.randn(48, 64, generator=g) * 0.1
    for bad in (float("inf"), float("-inf"), float("nan")):
        xb = x.clone(); xb[0, 7, 1, 4] = bad
        assert torch.isnan(_fwd_only(ops, "f16x2", xb, w)).all()
        wb = w.clone(); wb[5, 9] = bad
        assert torch.isnan(_fwd_only(ops, "f16x2", x, wb)).all()
    assert torch.isfinite(_fwd_only(ops, "f16x2", x, w)).all()
    # all-zero operands: zero result, no NaN from the scale
    assert (_fwd_only(ops, "f16x2", torch.zeros_like(x), w) == 0).all()
    assert (_fwd_only(ops, "f16x2", x, torch.zeros_like(w)) == 0).all()


def test_amax_partials(ops):
    """The reduction feeding the f16x2 scale: maximum of the words = max |x|, on contiguous tensors,
    channel-sliced views, sizes that are not multiples of four, and with a NaN inside."""
    g = torch.Generator().manual_seed(9)
    for shape in ((2, 5, 7, 9), (3, 64, 32, 64), (1, 1, 1, 1)):
        x = torch.randn(*shape, generator=g).cuda()
        p = ops._amax_partials(x)
        assert p.shape == (ops.AMAX_PARTIALS,) and p.dtype == torch.int32
        got = p.max().view(1).view(torch.float32)
        assert float(got) == float(x.abs().max())
    base = torch.randn(2, 12, 8, 16, generator=g).cuda()
    base[:, 8:] *= 100.0
    view = base[:, 2:8]                       # channel slice: batch stride != C H W
    assert float(ops._amax_partials(view).max().view(1).view(torch.float32)) == float(view.abs().max())
    base[1, 3, 2, 2] = float("nan")
    assert torch.isnan(ops._amax_partials(view).max().view(1).view(torch.float32)).all()


@pytest.mark.parametrize("scheme", SPLIT_SCHEMES)
def test_split_random_ragged_shapes(ops, scheme):
    """30 random small shapes (every combination of ragged M / K / N tiles, K < 8, N < 32, N % 16 != 0 for
    which the weight gradient takes the exact kernel): all four results within 2e-6 of fp64."""
    g = torch.Generator().manual_seed(2024)
    for case in range(30):
        B = int(torch.randint(1, 4, (1,), generator=g))
        Ci = int(torch.randint(1, 300, (1,), generator=g))
        Co = int(torch.randint(1, 300, (1,), generator=g))
        H = int(torch.randint(1, 24, (1,), generator=g))
        W = int(torch.randint(1, 40, (1,), generator=g))
        x = torch.randn(B, Ci, H, W, generator=g)
        w = torch.randn(Co, Ci, generator=g) * Ci ** -0.5
        b = torch.randn(Co, generator=g) * 0.1
        res = torch.randn(B, Co, H, W, generator=g)
        ct = torch.randn(B, Co, H, W, generator=g)
        ref = _fp64(x, w, b, res, ct, "SiLU")
        got = _run(ops, scheme, x, w, b, res, ct, "SiLU")
        for name, a, r in zip(("y", "gx", "gw", "gb"), got, ref):
            assert torch.isfinite(a).all(), (case, name)
            assert _err(a, r) <= 2e-6, (case, (B, Ci, Co, H, W), name, _err(a, r))


def test_batched_gemm_split_vs_exact():
    """paradis_bgemm (Newton-Schulz products of Muon) in both arithmetics against fp64."""
    from paradis_model_amd._lib import dptr, lib, stream_ptr
    g = torch.Generator().manual_seed(5)
    for (T, M, K, N) in [(3, 96, 160, 96), (2, 130, 130, 258), (5, 64, 64, 64), (1, 896, 1152, 896)]:
        A = (torch.randn(T, M, K, generator=g) * K ** -0.5).cuda()
        Bm = torch.randn(T, K, N, generator=g).cuda()
        ref = A.double() @ Bm.double()
        errs = {}
        for split in (False, True):
            C = torch.empty(T, M, N, device="cuda")
            ws = torch.empty(T * lib.paradis_pw_gemm_split_bytes(M, K, 3), dtype=torch.uint8, device="cuda") if split else None
            rc = lib.paradis_bgemm(dptr(A), None, dptr(Bm), dptr(C), T, M, K, N, M * K, 0, K * N, M * N,
                                   dptr(ws), stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            errs[split] = _err(C, ref)
        assert errs[True] <= 1.25 * errs[False] + 1e-7 and errs[True] <= 2e-6, ((T, M, K, N), errs)


def _fwd_only(ops, scheme, x, w):
    if isinstance(scheme, bool):
        scheme = "bf16x3" if scheme else "exact"
    keep = ops.GEMM_SCHEME
    ops.GEMM_SCHEME = ops._SCHEMES[scheme]
    try:
        with torch.no_grad():
            return ops.pointwise(x.cuda(), w.cuda()).cpu()
    finally:
        ops.GEMM_SCHEME = keep


def test_split_extreme_magnitudes(ops):
    """Edge semantics of the bf16 h/m/l split next to the exact f32 kernel (documented in DESIGN.md 4.1b):
      * operands of magnitude 1e+-30 whose products are O(1): fp32-level result (bf16 has fp32's exponent
        range, nothing over- or underflows in the split);
      * operands below ~1e-33: the m / l terms (2^-8, 2^-16 of the operand) fall below fp32's smallest
        normal number and are flushed - the split degrades gracefully towards bf16 precision of THAT
        operand (<= 2^-15 at 1e-35, <= 2^-7 at 1e-37..1e-38), where the exact kernel keeps fp32 precision.
        Activations and gradients of this model sit 20+ decades above that; PARADIS_GEMM=exact is the
        answer for data that does not;
      * |x| within half a bf16 ulp of FLT_MAX (>= 3.39e38) rounds to +-inf in the leading term: such an
        operand gives NaN where the exact kernel may still be finite;
      * Inf / NaN operands: every output they touch is non-finite in both arithmetics (the split turns
        Inf into NaN: Inf - Inf in the residual), every other output is untouched."""
    g = torch.Generator().manual_seed(77)
    B, Ci, Co, H, W = 1, 64, 48, 8, 16
    base_x = torch.randn(B, Ci, H, W, generator=g)
    base_w = torch.randn(Co, Ci, generator=g) * Ci ** -0.5
    ref = torch.einsum("oc,bchw->bohw", base_w.double(), base_x.double())
    for sx, sw in ((1e30, 1e-30), (1e-30, 1e30)):
        x, w = base_x * sx, base_w * sw
        want = torch.einsum("oc,bchw->bohw", w.double(), x.double())
        ys, ye = _fwd_only(ops, True, x, w), _fwd_only(ops, False, x, w)
        assert torch.isfinite(ys).all()
        es, ee = _err(ys, want), _err(ye, want)
        assert es <= 1.25 * ee + 1e-7 and es <= 2e-6, (sx, es, ee)
    # subnormal low terms of a tiny operand: graceful loss of its low bits, never garbage
    for tiny, bound in ((1e-35, 2.0 ** -15), (1e-37, 2.0 ** -7)):
        for x, w in ((base_x * tiny, base_w / tiny), (base_x / tiny * 1e-2, base_w * tiny * 1e2)):
            want = torch.einsum("oc,bchw->bohw", w.double(), x.double())
            ys = _fwd_only(ops, True, x, w)
            assert torch.isfinite(ys).all() and _err(ys, want) <= bound, (tiny, _err(ys, want))
    # the top half-ulp of the fp32 range
    x = base_x.clone()
    x[0, 3, 2, 5] = 3.0e38
    w = base_w * 1e-38
    ys, ye = _fwd_only(ops, True, x, w), _fwd_only(ops, False, x, w)
    assert torch.isfinite(ys).all() and torch.isfinite(ye).all()
    x[0, 3, 2, 5] = 3.4e38              # rounds to +inf as a bf16 leading term
    ys, ye = _fwd_only(ops, True, x, w), _fwd_only(ops, False, x, w)
    assert torch.isfinite(ye).all() and not torch.isfinite(ys[0, :, 2, 5]).any()
    # Inf and NaN operands: same set of non-finite outputs in both arithmetics
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = base_x.clone()
        x[0, 7, 1, 4] = bad
        ys, ye = _fwd_only(ops, True, x, base_w), _fwd_only(ops, False, x, base_w)
        assert torch.equal(torch.isfinite(ys), torch.isfinite(ye)), bad
        assert not torch.isfinite(ys[0, :, 1, 4]).any()
        keep = torch.isfinite(ys)
        assert float((ys[keep].double() - ref[keep]).abs().max() / ref.abs().max()) <= 2e-6
        w = base_w.clone()
        w[5, 9] = bad
        ys, ye = _fwd_only(ops, True, base_x, w), _fwd_only(ops, False, base_x, w)
        assert torch.equal(torch.isfinite(ys), torch.isfinite(ye)), bad
        assert not torch.isfinite(ys[0, 5]).any() and torch.isfinite(ys[0, :5]).all()


def test_f16x2_is_opt_in_and_traceable(ops):
    """The default arithmetic is bf16x3; f16x2 is chosen per call (``scheme=``) or through ``ops.GEMM_SCHEME`` and
    is an explicit integer argument of the ops, so its amax words are ordinary op outputs / inputs (no tensor
    attributes): forward under ``torch.inference_mode()`` works, and a gradient step with it equals one whose
    operands were scaled by read passes anyway (there is no other path any more)."""
    assert ops._scheme_from_env.__defaults__ is None
    import os
    if "PARADIS_GEMM" not in os.environ:
        assert ops.GEMM_SCHEME == ops.GEMM_BF16X3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 16, 32, generator=g).cuda()
    w = (torch.randn(48, 64, generator=g) * 0.1).cuda()
    want = torch.einsum("oc,bchw->bohw", w.double(), x.double())
    with torch.inference_mode():
        for scheme in (ops.GEMM_F16X2, ops.GEMM_BF16X3, ops.GEMM_EXACT):
            y = ops.pointwise(x, w, scheme=scheme)
            assert _err(y.cpu(), want.cpu()) <= 2e-6
    wr, xr = w.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ops.pointwise(xr, wr, act="SiLU", scheme=ops.GEMM_F16X2).square().sum().backward()
    wd, xd = w.double().requires_grad_(True), x.double().requires_grad_(True)
    torch.nn.functional.silu(torch.einsum("oc,bchw->bohw", wd, xd)).square().sum().backward()
    assert _err(wr.grad.cpu(), wd.grad.cpu()) <= 2e-6 and _err(xr.grad.cpu(), xd.grad.cpu()) <= 2e-6


# ---------------------------------------------------------------------------------------------------------------
# Round 5: direct tests of the bf16 MFMA's accumulator-alignment offset and of its remedy, the sign checkerboard
# (csrc/gemm_common.h "sign checkerboard").  Until round 5 only a 200-600 s model-level gradient
# test guarded against its return.
#
# What is measured (tools/gemm_bias_check.py, N(0,1) operands, unit u = 2^-24 rms(reference)): a six-product bf16 GEMM
# WITHOUT the checkerboard (-DSPLIT_SIGNED=0) carries the same offset on every output: mean signed error -0.9 u
# (y, dX) and -8 u (dW, 32,768-term sums) under 8 / 14 u of zero-mean noise; the f32 MFMA: +0.002 u.  With the
# checkerboard the plain mean is 0.000 u (dW: -0.006 u).  These tests fail on a -DSPLIT_SIGNED=0 build
# (verified on the GPU box with tools/build_variant.sh nosign "gemm_split.hip gemm_amp_fwd.hip gemm_amp_wgrad.hip" "-DSPLIT_SIGNED=0").
# Reference sums that exposed it: reference model/blocks.py:129-133 (ChannelNorm statistics and parameter gradients).
# ---------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = [(1024, 186), (384, 1024), (1536, 384), (768, 1024), (1024, 768), (1024, 1024), (896, 1152),
                (896, 896), (1024, 896), (768, 768), (97, 768)]       # (Co, Ci) of the default model
BIAS_GRIDS = [(32, 64, 4), (128, 256, 1)]                             # (H, W, B)


def _signed(got, ref):
    """(mean, rms, n) of the signed error in units of u = 2^-24 rms(ref)"""
    err = got.double() - ref
    u = float(ref.pow(2).mean().sqrt()) * 2.0 ** -24
    return float(err.mean()) / u, float(err.pow(2).mean().sqrt()) / u, err.numel()


def _gemm_triplet(ops, scheme, x, w, ct):
    xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = ops.pointwise(xx, ww, None, scheme=scheme)
    y.backward(ct)
    return y.detach(), xx.grad, ww.grad


@pytest.mark.parametrize("H,W,B", BIAS_GRIDS)
@pytest.mark.parametrize("Co,Ci", LAYER_SHAPES)
def test_mean_signed_error_of_every_layer_shape(ops, Co, Ci, H, W, B):
    """|mean signed error| of y, dX, dW against fp64 <= 0.1 u (+ the sampling noise of the mean, 4 rms / sqrt(n): it
    matters only for the 74,496-element dW of the 97-row output layer) for bf16x3 AND the f32-MFMA kernels, on N(0,1)
    operands, for every layer shape on both grids.  A -DSPLIT_SIGNED=0 build gives -0.9 u (y, dX) and up to -8 u (dW)."""
    g = torch.Generator().manual_seed(1000 + Co + Ci)
    x = torch.randn(B, Ci, H, W, generator=g).cuda()
    w = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).cuda()
    ct = torch.randn(B, Co, H, W, generator=g).cuda()
    xd, wd, cd = x.double(), w.double(), ct.double()
    refs = (torch.einsum("oc,bchw->bohw", wd, xd), torch.einsum("oc,bohw->bchw", wd, cd),
            torch.einsum("bohw,bchw->oc", cd, xd))
    del xd, wd, cd
    for name, scheme in (("bf16x3", ops.GEMM_BF16X3), ("exact", ops.GEMM_EXACT)):
        for what, got, ref in zip(("y", "dX", "dW"), _gemm_triplet(ops, scheme, x, w, ct), refs):
            mean, rms, n = _signed(got, ref)
            assert abs(mean) <= 0.1 + 4.0 * rms / n ** 0.5, (name, what, (Co, Ci), mean, rms)
            assert rms <= 40.0, (name, what, rms)          # (8-16 u measured: a plain sanity bound)


@pytest.mark.parametrize("Co,Ci", [(1536, 384), (1024, 1024)])
def test_weight_gradient_offset_cancels_between_slabs(ops, Co, Ci):
    """dW of the shape whose natural slab count is odd (1536 x 384: 21 -> 20) next to an even one: mean signed error
    within 0.1 u, rms not above 1.25 x the f32-MFMA kernel's."""
    g = torch.Generator().manual_seed(77)
    B, H, W = 4, 32, 64
    x = torch.randn(B, Ci, H, W, generator=g).cuda()
    w = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).cuda()
    ct = torch.randn(B, Co, H, W, generator=g).cuda()
    ref = torch.einsum("bohw,bchw->oc", ct.double(), x.double())
    m3, r3, n = _signed(_gemm_triplet(ops, ops.GEMM_BF16X3, x, w, ct)[2], ref)
    me, re_, _ = _signed(_gemm_triplet(ops, ops.GEMM_EXACT, x, w, ct)[2], ref)
    assert abs(m3) <= 0.1 + 4.0 * r3 / n ** 0.5 and abs(me) <= 0.1 + 4.0 * re_ / n ** 0.5, (m3, me)
    assert r3 <= 1.25 * re_, (r3, re_)


def test_pixel_and_channel_sums_of_a_gemm_output(ops):
    """The sums that exposed the offset (reference model/blocks.py:129-133: per-pixel channel statistics, parameter
    gradients summed over 32,768 pixels): row sums over the 32,768 pixels and column sums over the channels of y and dX
    at 128 x 256, accumulated in fp64 from the fp32 outputs, against the same sums of the fp64 product.  Error (rms over
    the sums) of bf16x3 <= 1.5 x the f32-MFMA kernel's.  A -DSPLIT_SIGNED=0 build: the 32,768-pixel sums carry
    0.9 u x 32,768 against 8 u x 181 of noise = 20 x.
    Sums over LESS than one 32-row x 64-column block see the offset with one sign (it is still there per element): over
    one 64-pixel run of one channel the bound is the offset plus the noise, 0.9 u x 64 + 8 u x 8 against 8 u x 8: the
    checkerboard cannot help there and 2.5 x is asserted (measured ~1.3 x)."""
    g = torch.Generator().manual_seed(5)
    B, H, W, Co, Ci = 1, 128, 256, 1024, 1024
    x = torch.randn(B, Ci, H, W, generator=g).cuda()
    w = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).cuda()
    ct = torch.randn(B, Co, H, W, generator=g).cuda()
    refs = (torch.einsum("oc,bchw->bohw", w.double(), x.double()), torch.einsum("oc,bohw->bchw", w.double(), ct.double()))
    out = {name: _gemm_triplet(ops, scheme, x, w, ct)[:2]
           for name, scheme in (("bf16x3", ops.GEMM_BF16X3), ("exact", ops.GEMM_EXACT))}

    def sum_err(t, ref, dims):
        return float((t.double().sum(dims) - ref.sum(dims)).pow(2).mean().sqrt())

    def run_err(t, ref):          # sums over single 64-pixel runs (one row of one checkerboard block)
        return float((t.double().reshape(-1, 64).sum(1) - ref.reshape(-1, 64).sum(1)).pow(2).mean().sqrt())

    for i, what in enumerate(("y", "dX")):
        for dims, label in (((0, 2, 3), "pixel sums"), ((1,), "channel sums")):
            e3, ee = sum_err(out["bf16x3"][i], refs[i], dims), sum_err(out["exact"][i], refs[i], dims)
            assert e3 <= 1.5 * ee, (what, label, e3, ee)
        e3, ee = run_err(out["bf16x3"][i], refs[i]), run_err(out["exact"][i], refs[i])
        assert e3 <= 2.5 * ee, (what, "64-pixel runs", e3, ee)


def test_two_thread_backward_shares_no_hint_state(ops):
    """The hint "this forward's backward will need the image of W^T" is an argument of the pointwise op, not process
    state (round 4 passed it through a module global around the op call, which autograd's multi-threaded backward and
    checkpoint recomputation on other threads could observe half-set).  Two Python threads run forward + backward
    concurrently on their own streams, one with input gradients and one without: both get the single-threaded results."""
    import threading
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(256, 192, generator=g) / 192 ** 0.5).cuda().requires_grad_(True)
    xs = [torch.randn(2, 192, 16, 32, generator=g).cuda() for _ in range(2)]
    cts = [torch.randn(2, 256, 16, 32, generator=g).cuda() for _ in range(2)]
    assert not hasattr(ops, "_WANT_WT_IMAGE")

    def work(i, need_x, out):
        with torch.cuda.stream(torch.cuda.Stream()):
            for _ in range(20):
                x = xs[i].clone().requires_grad_(need_x)
                y = ops.pointwise(x, w, None, act="SiLU")
                gw, = torch.autograd.grad(y, [w], cts[i], retain_graph=need_x)
                gx = torch.autograd.grad(y, [x], cts[i])[0] if need_x else None
            torch.cuda.current_stream().synchronize()
            out[i] = (y.detach(), gw, gx)

    want, got = {}, {}
    for i, need in enumerate((True, False)):
        work(i, need, want)
    ths = [threading.Thread(target=work, args=(i, need, got)) for i, need in enumerate((True, False))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    torch.cuda.synchronize()
    for i in range(2):
        for a, b in zip(want[i], got[i]):
            assert (a is None and b is None) or torch.equal(a, b), i
