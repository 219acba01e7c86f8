"""AMSE loss without a GPU: the CPU restatement (tests/amse_oracle.py) against quadrature identities and the reference's
own code (golden g8_amse.pt), the ParadisLoss("amse") front end, build_val_loss, and the fake kernels of the new ops."""
import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import amse_oracle as O
from _util import assert_chk, load_golden, seeded
from paradis_model_amd import ops
from paradis_model_amd.config import reduced_config
from paradis_model_amd.loss import ParadisLoss, build_loss, build_val_loss


@pytest.mark.parametrize("n", [4, 9, 10, 17, 33, 65, 66])
def test_cc_weights_integrate_polynomials_exactly(n):
    x, w = O.cc_weights(n)
    assert abs(w.sum() - 2.0) < 1e-14
    for d in range(n):
        exact = 0.0 if d % 2 else 2.0 / (d + 1)
        assert abs((w * x ** d).sum() - exact) < 1e-13, d


@pytest.mark.parametrize("n", [3, 4, 5, 6, 9, 10, 66, 67, 258])
def test_closed_cosine_form_of_the_cc_weights_equals_waldvogels(n):
    """the form sht.hip's cc_nodes_kernel evaluates, at both parities of n (2k == n1 occurs for odd n only)"""
    x, w = O.cc_weights(n)
    xc, wc = O.cc_weights_cosine(n)
    assert float(np.abs(wc - w).max()) <= 1e-14
    assert float(np.abs(xc[::-1] - x).max()) <= 1e-14      # (the kernel's nodes run from the north pole)


@pytest.mark.parametrize("H", [9, 10, 66])
def test_matrix_dft_equals_the_fft_in_fp64(H):
    x = seeded(H, 2, 3, H, 2 * (H - 1)).double()
    a, b = O.sht(x), O.sht(x, dft="matrix")
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    with pytest.raises(ValueError):
        O.sht(x, dft="dct")


@pytest.mark.parametrize("H,B,C", O.EDGE_CASES)
def test_edge_case_inputs_are_well_conditioned_for_the_fp32_reference(H, B, C, record_property):
    """The inputs of tests/test_hip_amse_edges.py: the fp32 CPU evaluations (FFT and matrix DFT) are within a third of
    the GPU test's 1e-5 ceiling of fp64 in value and in the worst plane's gradient, so that test neither passes nor
    fails on the reference's own noise; every edge mode the design asks for is on some plane, and no two planes agree."""
    pred, target = O.edge_fields(H, B, C)
    N, W, em = B * C, 2 * (H - 1), O.edge_modes(H)
    assert pred.shape == target.shape == (B, C, H, W) and pred.dtype == torch.float32
    assert all(0 <= m <= l < H - 1 for l, m in em) and len(set(em)) == len(em)
    assert {(0, 0), (H - 2, 0), (H - 2, H - 2)} <= set(em)
    # the spikes stand out of the noise in the fp64 coefficients of the planes that carry them
    c = O.sht(target.view(N, H, W).double()).abs()
    floor = float(c[:, O._tri_mask(H)].median())
    for e, (l, m) in enumerate(em):
        carriers = [n for n in range(N) if any((n + 3 * j) % len(em) == e for j in range((len(em) + 2) // 3))]
        if l + l <= H - 1:      # (the quadrature returns a synthesised mode exactly where 2 l <= H - 1)
            assert all(float(c[n, l, m]) > 8 * floor for n in carriers[:4]), (l, m)
    flat = target.view(N, -1)
    assert N == 1 or float((flat[1:] - flat[:-1]).abs().amax(1).min()) > 0
    _, _, e_cpu = O.edge_reference(H, B, C)
    for k, v in e_cpu.items():
        record_property(f"e_cpu_{k}", v)
    print(f"amse edge {H, B, C}: e_cpu value {e_cpu['value']:.2e} grad {e_cpu['grad']:.2e} plane {e_cpu['plane']:.2e}")
    assert e_cpu["value"] <= 3.3e-6 and e_cpu["plane"] <= 3.3e-6, e_cpu


@pytest.mark.parametrize("n", [9, 33])
def test_table_is_discretely_orthogonal(n):
    tabs = O.tables(n)
    th = O.colatitudes(n)
    for m, tab in tabs.items():
        plain = O.legendre_order(m, n - 1, th)
        gram = tab @ plain.T          # sum_j w_j P_l P_l' = 4 pi / (2 pi) = 2 delta (sqrt(4 pi)-scaled functions)
        L = gram.shape[0]
        for a in range(L):
            for b in range(L):
                if (m + a) + (m + b) <= n - 1:
                    assert abs(gram[a, b] - (2.0 if a == b else 0.0)) < 1e-12, (m, a, b)


def test_synthesised_modes_come_back():
    H, W = 33, 64
    modes = {(3, 2): 1 + 2j, (5, 0): 0.5, (7, 7): -1j, (10, 1): 0.25 - 0.75j}
    c = O.sht(O.synth(H, W, modes)[None, None])[0, 0]
    lcut = H - 1 - max(l for l, _ in modes)
    want = torch.zeros_like(c)
    for (l, m), v in modes.items():
        want[l, m] = v
    assert float((c[:lcut + 1] - want[:lcut + 1]).abs().max()) < 1e-12


def test_oracle_equals_the_reference_golden():
    g = load_golden("g8_amse.pt")
    B, C = g["B"], g["C"]
    for case in g["cases"]:
        H, W, seed = case["H"], case["W"], case["seed"]
        t = seeded(seed, B, C, H, W)
        p = seeded(seed + 100, B, C, H, W) if case["regime"] == "independent" else t + 0.01 * seeded(seed + 200, B, C, H, W)
        assert_chk([p, t], case["chk"])
        pr = p.clone().requires_grad_(True)
        a32 = O.amse(pr, t, torch.float32)
        val = (a32 * case["feature_weights"].view(1, -1, 1, 1)).mean()
        val.backward()
        # fp32 against fp32 in another summation order: the near regime carries the cancellation in 1 - coh
        tol, gtol = (1e-5, 1e-4) if case["regime"] == "independent" else (3e-3, 1e-3)
        a = float(a32.detach())
        assert abs(a - case["amse"]) <= tol * abs(case["amse"]), case["regime"]
        assert abs(float(val.detach()) - case["loss"]) <= tol * abs(case["loss"])
        gs = pr.grad.reshape(-1)[::g["grad_stride"]]
        assert float((gs - case["grad_sub"]).abs().max() / case["grad_sub"].abs().max()) <= gtol
        pcl = a * case["feature_weights"]
        assert torch.allclose(pcl, case["per_channel"], rtol=tol, atol=0)


def _loss(kind, H=17, lat_weights=True):
    lat = torch.linspace(-90.0, 90.0, H, dtype=torch.float64)
    return ParadisLoss(kind, lat, torch.tensor([500.0, 850.0]), num_features=3, num_surface_vars=1,
                       var_loss_weights=torch.tensor([1.0, 0.5, 2.0]), output_name_order=["t_h0", "t_h1", "msl"],
                       apply_latitude_weights=lat_weights)


def test_paradis_loss_amse_constructs_and_disables_latitude_weights():
    loss = _loss("amse")
    assert loss.kind == "amse" and loss.apply_latitude_weights is False
    assert (loss.nlat, loss.nlon) == (17, 32)
    assert _loss("mse").apply_latitude_weights is True
    with pytest.raises(Exception, match=r"not supported, choose between \[reversed_huber, mse\]"):
        _loss("mae")


@pytest.mark.parametrize("H,W", [(32, 64), (128, 256), (17, 34), (2, 2)])
def test_grids_other_than_w_equals_2h_minus_2_raise(H, W):
    x = torch.zeros(1, 3, H, W)
    with pytest.raises(ValueError, match=r"nlon = 2\*\(nlat-1\)"):
        ops.amse_loss(x, x)
    if H > 2:
        loss = _loss("amse", H)
        with pytest.raises(ValueError, match=r"nlon = 2\*\(nlat-1\)"):
            loss(x, x)


def test_build_val_loss_mirrors_the_reference_trainer():
    cfg = reduced_config()
    lat = torch.linspace(-90.0, 90.0, 17)
    train = build_loss(cfg, lat)
    assert build_val_loss(cfg, lat, train) is train                 # no validation_loss: the training loss object
    assert build_val_loss(cfg, lat).kind == cfg.training.loss_function.type
    cfg.training.loss_function.validation_loss = "amse"
    val = build_val_loss(cfg, lat, train)
    assert val is not train and val.kind == "amse" and val.apply_latitude_weights is False
    assert torch.equal(val.feature_weights, train.feature_weights)
    cfg.training.loss_function.validation_loss = None
    assert build_val_loss(cfg, lat, train) is train
    cfg.training.loss_function.type = "amse"
    assert build_loss(cfg, lat).kind == "amse"


def test_amse_ops_are_registered_without_a_cpu_kernel():
    for name in ("amse_loss", "amse_tables"):
        assert name in ops.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"paradis::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"paradis::{name}", "CPU")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("paradis::amse_loss", "Autograd")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("paradis::amse_loss", "AutocastCUDA")


def test_fake_tensor_shapes_of_the_amse_ops():
    H, W = 33, 64
    M = H - 1
    with FakeTensorMode(allow_non_fake_inputs=True):
        like = torch.empty(0, device="cuda")
        leg, tw = torch.ops.paradis.amse_tables(like, H, W)
        assert leg.shape == (M * (M + 1) // 2 * H,) and tw.shape == (W, 2 * M)
        p = torch.empty(2, 5, H, W, device="cuda")
        loss, grad = torch.ops.paradis.amse_loss(p, p, leg, tw, True)
        assert loss.shape == () and grad.shape == p.shape and loss.device.type == "cuda"
        loss, grad = torch.ops.paradis.amse_loss(p, p, leg, tw, False)
        assert grad.numel() == 0
        x = torch.empty(2, 5, H, W, device="cuda", requires_grad=True)
        val = ops.amse_loss(x, p)
        assert val.shape == () and val.requires_grad
        assert ops.amse_loss(x.detach().to(torch.bfloat16), p).dtype == torch.float32     # widened, as the reference
    assert not ops._AMSE_TABLES, "a fake table must not be cached"
    assert np.isclose(O.SHT_NORM_FACTOR ** 2, 4 * np.pi)
