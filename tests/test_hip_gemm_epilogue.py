"""The compile-time epilogue of the six-product (bf16x3) forward / data-gradient GEMM against the run-time one.

Claim under test (csrc/gemm_split.hip, ``split_epilogue_interior``): for every option set that has its own instantiation
the interior tiles of a launch come out with the SAME BITS as ``gemm_epilogue`` gives them - same operations, same order,
same contraction per element - and everything without an instantiation (GELU here), like every ragged tile, still runs
``gemm_epilogue``.  ``PARADIS_GEMM_EPILOGUE=generic`` is read at every launch and forces the run-time epilogue, so both
paths run in this process on the same inputs; every comparison is bitwise (a NaN must come out as the same NaN).

Shapes: N = 256 is one full 128 x 256 tile with both halves live, N = 768 an odd number of 128-column tiles (the dead
second half of the last tile pair); Co (M) in {128, 256} with K in {32, 40} (ragged K, epilogue-dominated); and the mixed
launches - M = 97 (ragged M only), N = 180 (ragged N), M = 160 with N = 384 (an interior tile next to ragged ones) - in
which each tile takes its own path.  The data gradient runs the same kernel with the roles of Co and Ci exchanged, so its
cases give the OUTPUT (Ci) the tile-sized channel count."""
import contextlib
import os

import pytest
import torch

from tests._util import seeded

pytestmark = pytest.mark.gpu

# B, H, W, M (output channels of the GEMM under test), K (its reduction length)
SHAPES = [
    (1, 4, 64, 128, 32),
    (1, 4, 64, 256, 40),
    (3, 4, 64, 128, 40),
    (3, 4, 64, 256, 32),
    (1, 4, 64, 97, 32),       # ragged M: no interior tile
    (1, 5, 36, 128, 40),      # N = 180: ragged N
    (1, 6, 64, 160, 32),      # N = 384: interior tile (rows 0-127, columns 0-255) next to ragged ones
]
# forward option sets: (bias map, residual, gate, activation, saved pre-activation); the bias is always there
FWD = {
    "bias": (False, False, False, None, False),
    "bias+res": (False, True, False, None, False),
    "bias+res+gate": (False, True, True, None, False),
    "bias+SiLU+z": (False, False, False, "SiLU", True),
    "bias+map+res": (True, True, False, None, False),
    "bias+map+SiLU+z": (True, False, False, "SiLU", True),
    "bias+GELU+z (not instantiated)": (False, False, False, "GELU", True),
}
# data-gradient option sets: activation whose gradient is applied from the producer's pre-activation
DGRAD = {"plain": None, "SiLU'": "SiLU", "GELU' (not instantiated)": "GELU"}


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


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _tails(seed, *shape):
    """values on both sides of 0, a tenth of them spread out to +-30 (the tails of SiLU and of its derivative)"""
    t = seeded(seed, *shape)
    wide = seeded(seed + 1, *shape, scale=30.0, kind="uniform")
    pick = seeded(seed + 2, *shape, kind="uniform") > 0.8
    return torch.where(pick, wide, t)


@pytest.fixture(scope="module")
def inputs():
    """seeded inputs per shape, made once and shared by every option set (nothing writes to them)"""
    out = {}
    for i, (B, H, W, M, K) in enumerate(SHAPES):
        s = 100 * i
        x = seeded(s + 1, B, K, H, W, scale=8.0)       # W x + b spreads over the SiLU tails as well
        x[0, 0, 0, 1] = float("nan")                     # one pixel of sample 0 becomes NaN in every output channel
        out[(B, H, W, M, K)] = {
            "x": x.cuda(), "w": (seeded(s + 2, M, K, 1, 1) / K ** 0.5).cuda(), "b": seeded(s + 3, M).cuda(),
            "map": seeded(s + 4, M, H, W).cuda(), "res": _tails(s + 5, B, M, H, W).cuda(), "gate": seeded(s + 8, M, scale=2.0).cuda(),
            # data gradient: dz [B, K, H, W] through weight [K, M] gives dx [B, M, H, W]; zpre = the producer's pre-activation
            "dz": seeded(s + 9, B, K, H, W).cuda(), "wd": (seeded(s + 10, K, M, 1, 1) / K ** 0.5).cuda(),
            "zpre": _tails(s + 11, B, M, H, W).cuda(),
        }
        out[(B, H, W, M, K)]["dz"][0, 0, 0, 2] = float("nan")
    return out


def _forward(ops, d, name):
    from paradis_model_amd.ops._core import ACT_CODES
    from paradis_model_amd.ops.gemm import _pointwise
    use_map, use_res, use_gate, act, save_z = FWD[name]
    y, z, _ = _pointwise(d["x"], d["w"], d["b"], d["map"] if use_map else None, d["res"] if use_res else None,
                         ACT_CODES[act], None, 0, False, None, None, save_z, ops._SCHEMES["bf16x3"],
                         d["gate"] if use_gate else None)
    torch.cuda.synchronize()
    return y, z


@pytest.mark.parametrize("name", list(FWD))
@pytest.mark.parametrize("B,H,W,M,K", SHAPES)
def test_forward_matches_the_generic_epilogue_bitwise(ops, inputs, B, H, W, M, K, name):
    d = inputs[(B, H, W, M, K)]
    y, z = _forward(ops, d, name)
    with _generic_epilogue():
        y_ref, z_ref = _forward(ops, d, name)
    assert _same_bits(y, y_ref), "y differs in %d elements" % int((y.view(torch.int32) != y_ref.view(torch.int32)).sum())
    assert _same_bits(z, z_ref), "saved z differs"
    assert z.numel() == (y.numel() if FWD[name][4] else 0)
    nan = torch.isnan(y)
    assert bool(nan[0, :, 0, 1].all()) and int(nan.sum()) == M      # the NaN pixel, and nothing else


@pytest.mark.parametrize("name", list(DGRAD))
@pytest.mark.parametrize("B,H,W,M,K", SHAPES)
def test_data_gradient_matches_the_generic_epilogue_bitwise(ops, inputs, B, H, W, M, K, name):
    from paradis_model_amd.ops._core import ACT_CODES
    from paradis_model_amd.ops.gemm import _pw_gemm_dgrad
    d = inputs[(B, H, W, M, K)]
    act = ACT_CODES[DGRAD[name]]

    def run():
        dx = _pw_gemm_dgrad(d["dz"], d["wd"], d["zpre"] if act else None, act, None, ops._SCHEMES["bf16x3"])
        torch.cuda.synchronize()
        return dx

    dx = run()
    with _generic_epilogue():
        dx_ref = run()
    assert dx.shape == (B, M, H, W)
    assert _same_bits(dx, dx_ref), "dX differs in %d elements" % int((dx.view(torch.int32) != dx_ref.view(torch.int32)).sum())
    assert bool(torch.isnan(dx[0, :, 0, 2]).all()) and int(torch.isnan(dx).sum()) == M


@pytest.mark.parametrize("B,H,W,M,K", SHAPES)
def test_weight_and_bias_gradient_do_not_depend_on_the_switch(ops, inputs, B, H, W, M, K):
    """dW and db come from the weight-gradient kernel, which keeps its epilogue: the same bits under either setting"""
    from paradis_model_amd.ops.gemm import _pw_gemm_wgrad
    d = inputs[(B, H, W, M, K)]
    dy = d["res"]                                       # [B, M, H, W]: any finite cotangent
    x = torch.nan_to_num(d["x"], nan=0.5)

    def run():
        gw, gb = _pw_gemm_wgrad(dy, x, True, None, None, ops._SCHEMES["bf16x3"])
        torch.cuda.synchronize()
        return gw, gb

    gw, gb = run()
    with _generic_epilogue():
        gw_ref, gb_ref = run()
    assert gw.shape == (M, K) and gb.shape == (M,)
    assert _same_bits(gw, gw_ref) and _same_bits(gb, gb_ref)
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())


@pytest.mark.parametrize("B,H,W,M,K", SHAPES[:4] + SHAPES[6:])
def test_gated_epilogue_is_gated_blend_of_the_plain_result(ops, inputs, B, H, W, M, K):
    """``NeuralSemiLagrangian.transport`` relies on it: pointwise(..., residual=h, gate=alpha) carries the bits of
    gated_blend(h, pointwise(...), alpha)"""
    d = inputs[(B, H, W, M, K)]
    x = torch.nan_to_num(d["x"], nan=-0.25)
    with torch.no_grad():
        fused = ops.pointwise(x, d["w"], d["b"], residual=d["res"], gate=d["gate"], scheme=ops._SCHEMES["bf16x3"])
        two_pass = ops.gated_blend(d["res"], ops.pointwise(x, d["w"], d["b"], scheme=ops._SCHEMES["bf16x3"]), d["gate"])
        with _generic_epilogue():
            fused_generic = ops.pointwise(x, d["w"], d["b"], residual=d["res"], gate=d["gate"], scheme=ops._SCHEMES["bf16x3"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fused).all())
    assert _same_bits(fused, two_pass)
    assert _same_bits(fused, fused_generic)
