"""GPU: the AMSE loss (sht.hip through ops.amse_loss / ParadisLoss("amse")) against the fp64 CPU restatement
(tests/amse_oracle.py) and the reference's own code (golden g8_amse.pt): tables, value, gradient, NaN / empty handling,
determinism, and the loss inside the training step (eager, graphed, bf16-mixed) and the validation path."""
import numpy as np
import pytest
import torch

import amse_oracle as O
from _util import load_golden, make_grid, max_rel, seeded

pytestmark = pytest.mark.gpu


def _ops():
    from paradis_model_amd import ops
    return ops


def _tri(m, M):
    return m * M - m * (m - 1) // 2


def _check_tables(H, ms):
    W = 2 * (H - 1)
    M = H - 1
    leg, tw = _ops().amse_tables(H, W, "cuda")
    leg = leg.cpu().double()
    ref = O.tables(H, ms)
    for m in ms:
        got = leg[_tri(m, M) * H:(_tri(m, M) + M - m) * H].view(M - m, H)
        r = torch.from_numpy(ref[m])
        assert float((got - r).abs().max()) <= 2e-7 * float(r.abs().max()) + 1e-30, (H, m)
    i = np.arange(W)[:, None]
    mm = np.arange(M)[None, :]
    ang = 2 * np.pi * ((i * mm) % W) / W
    twr = torch.from_numpy(np.concatenate([np.cos(ang), -np.sin(ang)], 1) * 2 * np.pi / W)
    assert float((tw.cpu().double() - twr).abs().max()) <= 1e-7 * 2 * np.pi / W


@pytest.mark.parametrize("H", [9, 17, 33, 129])
def test_tables_match_the_oracle(H):
    _check_tables(H, range(H - 1))


def test_tables_match_the_oracle_at_721_on_an_order_subset():
    _check_tables(721, [0, 1, 2, 7, 64, 255, 360, 511, 700, 719])


def _pair(H, W, seed, regime, B=2, C=3):
    t = seeded(seed, B, C, H, W)
    if regime == "independent":
        return seeded(seed + 100, B, C, H, W), t
    return t + 0.01 * seeded(seed + 200, B, C, H, W), t


def _oracle(p, t, dtype):
    pr = p.to(dtype).clone().requires_grad_(True)
    v = O.amse(pr, t.to(dtype), dtype)
    v.backward()
    return float(v.detach()), pr.grad.double()


def _device(p, t, scale=1.0):
    pd = p.cuda().requires_grad_(True)
    v = _ops().amse_loss(pd, t.cuda())
    (v * scale).backward()
    return float(v.detach()), pd.grad.double().cpu()


@pytest.mark.parametrize("H", [9, 33, 65])
@pytest.mark.parametrize("regime", ["independent", "near"])
def test_value_and_gradient_against_fp64(H, regime):
    W = 2 * (H - 1)
    p, t = _pair(H, W, 3 + H, regime)
    v64, g64 = _oracle(p.double(), t.double(), torch.float64)
    v, g = _device(p, t)
    verr, gerr = abs(v - v64) / abs(v64), max_rel(g, g64)
    if regime == "independent":
        assert verr <= 1e-5 and gerr <= 1e-5, (verr, gerr)
    else:   # the fp32 reference path itself loses digits in 1 - coh here: at most 3x its own error
        v32, g32 = _oracle(p, t, torch.float32)
        vtol = max(3 * abs(v32 - v64) / abs(v64), 1e-6)
        gtol = max(3 * max_rel(g32, g64), 1e-6)
        assert verr <= vtol and gerr <= gtol, (verr, vtol, gerr, gtol)


def test_paradis_loss_amse_matches_the_reference_golden():
    from paradis_model_amd.loss import ParadisLoss
    g = load_golden("g8_amse.pt")
    for case in g["cases"]:
        H, W = case["H"], case["W"]
        p, t = _pair(H, W, case["seed"], case["regime"], g["B"], g["C"])
        loss = ParadisLoss("amse", torch.linspace(-90.0, 90.0, H, dtype=torch.float64), torch.tensor(g["levels"]),
                           num_features=g["C"], num_surface_vars=1, var_loss_weights=torch.tensor([1.0, 0.5, 2.0]),
                           output_name_order=["t_h0", "t_h1", "msl"], apply_latitude_weights=True).cuda()
        assert torch.equal(loss.feature_weights, case["feature_weights"])
        pd = p.cuda().requires_grad_(True)
        val = loss(pd, t.cuda())
        val.backward()
        tol, gtol = (1e-5, 1e-4) if case["regime"] == "independent" else (3e-3, 1e-3)
        assert abs(float(val.detach()) - case["loss"]) <= tol * abs(case["loss"]), case["regime"]
        gs = pd.grad.cpu().reshape(-1)[::g["grad_stride"]]
        assert max_rel(gs, case["grad_sub"]) <= gtol
        with torch.no_grad():
            pcl = loss.per_channel_loss(p.cuda(), t.cuda()).cpu()
        assert torch.allclose(pcl, case["per_channel"], rtol=tol, atol=0)


def test_upstream_scale_no_grad_and_bitwise_repeats():
    ops = _ops()
    H, W = 33, 64
    p, t = _pair(H, W, 7, "independent")
    v1, g1 = _device(p, t, 1.0)
    v3, g3 = _device(p, t, 3.0)
    assert v1 == v3
    assert max_rel(g3, 3 * g1) <= 1e-6
    v1b, g1b = _device(p, t, 1.0)
    assert v1b == v1 and torch.equal(g1b, g1)
    leg, tw = ops.amse_tables(H, W, "cuda")
    with torch.no_grad():
        val, grad = torch.ops.paradis.amse_loss(p.cuda(), t.cuda(), leg, tw, False)
    assert grad.numel() == 0 and float(val) == v1
    pd = p.cuda().requires_grad_(True)
    with torch.no_grad():
        v = ops.amse_loss(pd, t.cuda())
    assert not v.requires_grad
    with torch.autocast("cuda", dtype=torch.bfloat16):
        vb = ops.amse_loss(p.cuda().bfloat16(), t.cuda().bfloat16())
    assert vb.dtype == torch.float32
    assert abs(float(vb) - float(ops.amse_loss(p.bfloat16().float().cuda(), t.bfloat16().float().cuda()))) == 0.0


def test_empty_batch_and_nan_give_1e6_with_zero_gradient_without_a_host_sync():
    ops = _ops()
    H, W = 17, 32
    p, t = _pair(H, W, 9, "independent")
    p[0, 1, 3, 5] = float("nan")
    pe = torch.zeros(0, 3, H, W, device="cuda", requires_grad=True)
    pd = p.cuda().requires_grad_(True)
    td = t.cuda()
    ops.amse_tables(H, W, "cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ve = ops.amse_loss(pe, td[:0])
        ve.backward()
        vn = ops.amse_loss(pd, td)
        vn.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert float(ve) == 1e6 and pe.grad.shape == pe.shape
    assert float(vn) == 1e6
    assert torch.equal(pd.grad, torch.zeros_like(pd.grad))


def _train_setup(loss_type, capturable=False, amp=False):
    from paradis_model_amd.config import reduced_config, stub_datamodule
    from paradis_model_amd.harness import TrainStep, synthetic_batch
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = reduced_config()
    cfg.training.loss_function.type = loss_type
    lat_deg, lg, og = make_grid(17, 32, True)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda()
    lat64 = torch.linspace(-90.0, 90.0, 17, dtype=torch.float64)
    step = TrainStep(model, build_loss(cfg, lat64).cuda(), cfg, capturable=capturable, amp=amp)
    batches = [synthetic_batch(17, 32, True, 2, 2, seed=5 + i, device="cuda") for i in range(2)]
    return cfg, lat64, model, step, batches


def test_train_step_with_amse_eager_equals_graphed_and_runs_under_amp():
    from paradis_model_amd.harness import GraphedTrainStep
    n_steps, warm = 4, 2
    _, _, model_e, step_e, batches = _train_setup("amse")
    order = [0] * warm + [i % 2 for i in range(n_steps - warm)]
    losses_e = [float(step_e(batches[i])) for i in order]
    _, _, model_g, step_g, _ = _train_setup("amse", capturable=True)
    g = GraphedTrainStep(step_g, batches[0], warmup=warm)
    losses_g = [float(g(batches[i])) for i in order[warm:]]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses_e)) and losses_e[0] != 1e6
    for a, b in zip(losses_e[warm:], losses_g):
        assert abs(a - b) <= 1e-6 * abs(a), (losses_e, losses_g)
    pe = torch.cat([p.detach().flatten() for p in model_e.parameters()])
    pg = torch.cat([p.detach().flatten() for p in model_g.parameters()])
    assert max_rel(pg, pe) <= 1e-6
    _, _, _, step_a, batches_a = _train_setup("amse", amp=True)
    la = [float(step_a(batches_a[0])) for _ in range(2)]
    assert all(np.isfinite(la)) and abs(la[0] - losses_e[0]) <= 0.1 * abs(losses_e[0])


def test_validation_loss_amse_under_inference_mode():
    from paradis_model_amd.loss import build_val_loss
    cfg, lat_deg, model, step, batches = _train_setup("reversed_huber")
    cfg.training.loss_function.validation_loss = "amse"
    val = build_val_loss(cfg, lat_deg, step.loss_fn).cuda()
    assert val.kind == "amse"
    p, t = _pair(17, 32, 4, "independent", 2, val.num_features)
    with torch.inference_mode():
        v = val(p.cuda(), t.cuda())
    ref = (O.amse(p.double(), t.double()) * val.feature_weights.double().view(1, -1, 1, 1)).mean()
    assert abs(float(v) - float(ref)) <= 1e-5 * abs(float(ref))


def test_full_resolution_call_is_finite_and_recovers_a_synthesised_mode():
    ops = _ops()
    H, W, C = 721, 1440, 97
    modes = {(40, 12): 1.5 - 0.5j}
    f = O.synth(H, W, modes).float()
    # channel c at the scale s_c = 1 + c / C, pred and target alike: the loss is homogeneous of degree 2 apart from the
    # eps floor, so the value is mean_c(s_c^2) times that of one channel and grad[c] = s_c grad[0]; a plane written to
    # the wrong channel shows
    s = 1.0 + torch.arange(C, dtype=torch.float32) / C
    p = (f.view(1, 1, H, W) * s.view(1, C, 1, 1)).contiguous().cuda().requires_grad_(True)
    t = (2.0 * p.detach()).contiguous()
    v = ops.amse_loss(p, t)
    v.backward()
    torch.cuda.synchronize()
    # pred's PSD at k = 40 is 2 |c|^2, the target's 4x that, coherence 1: amse_40 = 2|c|^2 (the rest sit at the eps floor)
    a = 2 * abs(1.5 - 0.5j) ** 2
    want = float((s.double() ** 2).mean()) * (a + (H - 2) * 0.0) / (H - 1)
    assert np.isfinite(float(v)) and abs(float(v) - want) <= 1e-3 * want, (float(v), want)
    assert bool(torch.isfinite(p.grad).all())
    g = p.grad[0].cpu()
    for c in range(C):
        assert max_rel(g[c], float(s[c]) * g[0]) <= 1e-3, c
