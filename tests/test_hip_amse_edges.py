"""GPU: the AMSE loss (csrc/sht.hip) against fp64 at every tile and block edge of its kernels.  All four transforms run
through one 64 x 64 x 16 GEMM (sht_gemm_kernel) under four index mappings:

    DftFwd   rows 2M (cos | sin)  cols H N        depth W
    LegFwd   rows M - m, per m    cols 4N         depth H
    LegAdj   rows H               cols 2N         depth M - m, per m
    DftAdj   rows H N             cols W          depth 2M

(M = H - 1, W = 2M, N = B C), amse_spectral_kernel takes 256 planes per block and amse_finish_kernel strides the planes
by 256.  The cases (amse_oracle.EDGE_CASES, the comment beside each names the branch it selects) are derived from those
dispatch conditions; the inputs (amse_oracle.edge_fields) are dense white noise with spectral spikes 32 times the noise
on the first and last row of each 64-row tile of an order's triangle, a different third of them on each plane, and
every plane at a scale of its own.  tests/test_amse_cpu.py holds the fp32 CPU reference's own error on these inputs
under a third of the ceiling.

For every case      e_hip = error against the fp64 oracle      of the value, of the whole gradient (max_rel) and of
the worst plane (max|g_n - g64_n| / max|g64_n|), and e_cpu, the larger of the same for the two fp32 CPU evaluations
(FFT and matrix DFT).  Asserted: (1) the ceilings of test_hip_amse.py for independent fields, 1e-5, on all three;
(2) e_hip <= max(3 e_cpu, 1e-6) on the value and the whole gradient (the rule of test_hip_amse.py's near regime);
(3) two calls agree bit for bit.  Every figure is printed (``-s``) and recorded as a property.

Then: planes do not see each other (a batched call against N single-plane calls, bit for bit), the workspace query
and the argument checks of the C ABI, and the tables at even H, at the smallest grids and past j = 256."""
import numpy as np
import pytest
import torch

import amse_oracle as O
from test_hip_amse import _check_tables

pytestmark = pytest.mark.gpu
CEIL = 1e-5


@pytest.fixture(scope="module")
def ops():
    from paradis_model_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from paradis_model_amd import _lib
    return _lib


def _device(ops, p, t):
    pd = p.cuda().requires_grad_(True)
    v = ops.amse_loss(pd, t.cuda())
    v.backward()
    return v.detach().cpu(), pd.grad.cpu()


@pytest.mark.parametrize("H,B,C", O.EDGE_CASES)
def test_value_and_gradient_against_fp64_at_tile_and_block_edges(ops, H, B, C, record_property):
    p, t = O.edge_fields(H, B, C)
    v64, g64, e_cpu = O.edge_reference(H, B, C)
    v, g = _device(ops, p, t)
    e_hip = O.errors(float(v), g, v64, g64)
    for k in ("value", "grad", "plane"):
        record_property(f"e_hip_{k}", e_hip[k])
        record_property(f"e_cpu_{k}", e_cpu[k])
    print(f"amse edge {H, B, C}: e_hip / e_cpu  value {e_hip['value']:.2e} / {e_cpu['value']:.2e}  "
          f"grad {e_hip['grad']:.2e} / {e_cpu['grad']:.2e}  plane {e_hip['plane']:.2e} / {e_cpu['plane']:.2e}")
    v2, g2 = _device(ops, p, t)
    assert torch.equal(v2, v) and torch.equal(g2, g)              # fixed-order sums, no float atomics
    assert e_hip["value"] <= CEIL and e_hip["grad"] <= CEIL and e_hip["plane"] <= CEIL, e_hip
    assert e_hip["value"] <= max(3 * e_cpu["value"], 1e-6), (e_hip, e_cpu)
    assert e_hip["grad"] <= max(3 * e_cpu["grad"], 1e-6), (e_hip, e_cpu)


# N a power of two: gscale = 1 / (K N) differs from the single-plane call's by an exact scaling; 4N = 64 is one LegFwd
# column tile, 4N = 256 four of them (and two LegAdj tiles), so plane n's columns sit at another place of another tile
@pytest.mark.parametrize("N", [16, 64])
def test_planes_are_independent_bit_for_bit(ops, N):
    """Every GEMM output is the same dot product in the same depth order wherever its column sits in a tile, and H = 9
    has no table entry near fp32's underflow (sin(pi / 8)^7 = 1e-3): plane n of the batched gradient times N is the
    gradient of the call on plane n alone, and the batched value is the mean of the N single values."""
    p, t = O.edge_fields(9, 1, N)
    v, g = _device(ops, p, t)
    singles = []
    for n in range(N):
        vn, gn = _device(ops, p[:, n:n + 1], t[:, n:n + 1])
        singles.append(float(vn))
        assert torch.equal(g[:, n:n + 1] * N, gn), n
    want = np.float32(np.mean(np.array(singles, dtype=np.float64)))
    assert abs(float(v) - float(want)) <= float(np.spacing(want)), (float(v), float(want))


# 4N = 68 (a ragged column tile); even H with a one-row second row tile
@pytest.mark.parametrize("H,B,C", [(9, 1, 17), (66, 1, 5)])
def test_workspace_is_what_the_query_says(ops, L, H, B, C):
    """a call through the C ABI on a workspace of exactly paradis_amse_ws_bytes leaves the 4096 canary bytes behind it
    alone and returns the bytes of the op (which sizes its own workspace from the same query)"""
    p, t = (x.cuda() for x in O.edge_fields(H, B, C))
    N, W = B * C, 2 * (H - 1)
    pd = p.clone().requires_grad_(True)
    want = ops.amse_loss(pd, t)
    want.backward()
    leg, tw = ops.amse_tables(H, W, "cuda")
    nbytes = L.lib.paradis_amse_ws_bytes(N, H)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    loss, grad = torch.full((), -7.0, device="cuda"), torch.full_like(p, -7.0)
    rc = L.lib.paradis_amse_loss(L.dptr(p), L.dptr(t), L.dptr(leg), L.dptr(tw), L.dptr(loss), L.dptr(grad), L.dptr(ws),
                                 N, H, W, L.stream_ptr())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    assert not bool((ws[:nbytes - 256] == 0xA5).all())            # (the call did use the workspace handed in)
    assert torch.equal(loss, want.detach()) and torch.equal(grad, pd.grad)


# (N, H, W): W != 2(H - 1); H = 2 (no degree left); H N > 65535 * 64 = the row tiles of one DftAdj launch
@pytest.mark.parametrize("N,H,W,msg", [(3, 9, 18, "W = 2*(H-1)"), (3, 2, 2, "W = 2*(H-1)"), (466034, 9, 16, "too large")])
def test_bad_arguments_are_rejected_before_any_launch(L, N, H, W, msg):
    """the argument checks precede every launch, so small dummy buffers suffice: rc 1, the reason in last_error, and no
    buffer touched"""
    buf = [torch.full((64,), -7.0, device="cuda") for _ in range(7)]
    rc = L.lib.paradis_amse_loss(*(L.dptr(b) for b in buf), N, H, W, L.stream_ptr())
    assert rc == 1 and "amse_loss" in L.last_error() and msg in L.last_error(), L.last_error()
    torch.cuda.synchronize()
    for b in buf:
        assert bool((b == -7.0).all())


# all orders: the smallest grid, even H (the other parity of the Clenshaw-Curtis rule: no 2k == n1 term), a second row
# tile, three row tiles
@pytest.mark.parametrize("H", [3, 4, 10, 66, 131])
def test_tables_match_the_oracle_at_even_and_edge_grids(H):
    _check_tables(H, range(H - 1))


def test_tables_match_the_oracle_past_the_first_block_of_latitudes():
    """H = 258 (even): j >= 256 is the second block of cc_nodes_kernel and legendre_table_kernel"""
    _check_tables(258, [0, 1, 2, 63, 64, 128, 255, 256])
