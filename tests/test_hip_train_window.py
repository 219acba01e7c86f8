"""GPU: several backward passes meeting one optimiser step - gradient accumulation (``accumulate_grad_batches``), global-norm
clipping (``gradient_clip_val``) and truncated BPTT (``detach_gradient_every``) in ``harness.TrainStep`` and
``harness.GraphedTrainStep`` (reference trainer.py:498-587, train.py:52-53), on the reduced model at 16x32, B = 2."""
import pytest
import torch

from paradis_model_amd.config import reduced_config, stub_datamodule
from tests._util import make_grid, max_rel

pytestmark = pytest.mark.gpu

EPS23 = 2.0 ** -23

# MEASURED (MI355X, this file's set-up; the figures are printed by the tests):
#   window of two micro-batches against one step on their concatenation, per tensor ||g_window - g_big|| / ||g_big||:
#   fp32 reorder noise (dropping the 1/N would give 1.0).
WINDOW_GRAD_MEASURED = 2.815e-7
WINDOW_GRAD_BOUND = 2 * WINDOW_GRAD_MEASURED
#   truncated BPTT (detach every step, S = 3) against the same gradients built from three single-step calls on the inputs
#   of a no-grad rollout, per tensor norm-wise.
TBPTT_GRAD_MEASURED = 0.0
TBPTT_GRAD_BOUND = 2 * TBPTT_GRAD_MEASURED


def _setup(capturable=False, optimizer="adamw", detach=None, stats=False, **kw):
    from paradis_model_amd.diagnostics import TrainStats
    from paradis_model_amd.harness import TrainStep
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = reduced_config()
    cfg.training.optimizer.name = optimizer
    cfg.training.optimizer.detach_gradient_every = detach
    lat_deg, lg, og = make_grid(16, 32, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda()
    loss = build_loss(cfg, lat_deg).cuda()
    if stats:
        kw["stats"] = TrainStats(model, loss, channel_losses=False)
    return model, loss, cfg, TrainStep(model, loss, cfg, capturable=capturable, **kw)


def _batches(n, S=2, B=2, first_seed=5):
    from paradis_model_amd.harness import synthetic_batch
    return [synthetic_batch(16, 32, False, B, S, seed=first_seed + i, device="cuda") for i in range(n)]


@pytest.fixture(scope="module")
def batches():
    return _batches(6)


def _flat(model):
    return torch.cat([p.detach().flatten() for p in model.parameters()])


def _grads(model):
    return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def _norm64(grads):
    return float(sum(g.double().square().sum() for g in grads if g is not None).sqrt())


def _rel_per_tensor(got, ref):
    """worst norm-wise relative difference over the tensors"""
    worst = 0.0
    for a, b in zip(got, ref):
        assert (a is None) == (b is None)
        if b is None:
            continue
        nb = float(b.double().norm())
        d = float((a.double() - b.double()).norm())
        worst = max(worst, d / nb if nb > 0 else (0.0 if d == 0 else float("inf")))
    return worst


def _hand_loop(model, loss_fn, cfg, batches, N=1):
    """zero_grad / rollout_loss(accum=N) / optim.AdamW.step with the hyper-parameters of ``TrainStep``"""
    from paradis_model_amd.harness import rollout_loss
    from paradis_model_amd.optim import AdamW
    o = cfg.training.optimizer
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=o.lr, weight_decay=o.weight_decay,
                betas=(o.beta1, o.beta2))
    losses = []
    for k, b in enumerate(batches):
        if k % N == 0:
            opt.zero_grad(set_to_none=True)
        loss, _ = rollout_loss(model, loss_fn, b, num_common=83, n_inputs=2, accum=N)
        losses.append(loss)
        if (k + 1) % N == 0:
            opt.step()
    return losses


# ================================================================================================ 1. defaults
def test_defaults_change_nothing(batches):
    model, loss_fn, cfg, step = _setup()
    assert step.accumulate == 1 and step.clip_val is None
    losses = [step(b) for b in batches[:3]]
    ref, ref_loss, ref_cfg, _ = _setup()
    ref_losses = _hand_loop(ref, ref_loss, ref_cfg, batches[:3])
    assert torch.equal(_flat(model), _flat(ref))
    assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses))
    assert step.last_grad_norm is None and step.pending == 0 and step.opt_steps == 3


# ================================================================================================ 2. the window, exactly
def test_window_of_three_equals_the_hand_loop(batches):
    model, loss_fn, cfg, step = _setup(accumulate_grad_batches=3)
    pend = []
    for b in batches:
        step(b)
        pend.append(step.pending)
    assert pend == [1, 2, 0, 1, 2, 0] and step.opt_steps == 2
    ref, ref_loss, ref_cfg, _ = _setup()
    _hand_loop(ref, ref_loss, ref_cfg, batches, N=3)
    assert torch.equal(_flat(model), _flat(ref))
    # (AdamW is invariant to the scale of the gradient up to eps: only the exact comparison pins the 1/N)
    st = step.opt.state[next(iter(model.parameters()))]
    assert int(st["step"]) == 2


# ================================================================================================ 3. window = big batch
def _window_vs_big_batch():
    big = _batches(1, S=1, B=4)[0]
    halves = [tuple(t[i * 2:(i + 1) * 2].contiguous() for t in big) for i in range(2)]
    model_w, _, _, step_w = _setup(accumulate_grad_batches=2)
    model_b, _, _, step_b = _setup()
    p0 = _flat(model_w).clone()
    lw = step_w.window(halves)
    lb = step_b(big)
    torch.cuda.synchronize()
    return dict(loss_window=float(lw.mean()), loss_big=float(lb), grad=_rel_per_tensor(_grads(model_w), _grads(model_b)),
                pw=_flat(model_w), pb=_flat(model_b), p0=p0)


def test_window_of_two_equals_one_step_on_the_concatenation():
    r = _window_vs_big_batch()
    d = (r["pw"] - r["pb"]).abs()
    print("MEASURED | window of two vs big batch | gradients per tensor %.3e | losses %.3e | parameters max %.3e mean %.3e"
          % (r["grad"], abs(r["loss_window"] - r["loss_big"]) / abs(r["loss_big"]), float(d.max()), float(d.mean())))
    assert abs(r["loss_window"] - r["loss_big"]) <= 1e-5 * abs(r["loss_big"])
    assert float(d.max()) < 5e-4 and float(d.mean()) < 2e-5
    assert float((r["pw"] - r["p0"]).abs().max()) > 1e-5          # the step did move the parameters
    assert r["grad"] <= WINDOW_GRAD_BOUND, r["grad"]
    assert WINDOW_GRAD_BOUND < 1e-3                                 # orders below the 1.0 of a dropped 1/N


# ================================================================================================ 4. clipping in the step
@pytest.mark.parametrize("optimizer", ["adamw", "normuon"])
def test_clipping_in_the_step(optimizer, batches):
    """An unclipped twin gives norm64 of its gradients.  With ``gradient_clip_val`` = norm64 / 2: ``last_grad_norm[0]`` within
    2^-23 of norm64, ``p.grad`` bit-equal to the twin's gradient times the coefficient, the parameters bit-equal to a twin
    whose gradients were ``mul_``-ed by that coefficient before its ``opt.step()``; with 2 norm64: the parameters bit-equal to
    the unclipped twin.

    NorMuon: the norm sums of ``paradis_muon_step`` are reduced in a fixed order (csrc/muon.hip), so identical steps are
    bit-identical and the same equalities hold as for AdamW.  MEASURED (MI355X, one step, three pairs of runs): 0 of 118,587
    parameters differ between identical NorMuon runs and between the clipped step and its ``mul_`` twin (with float atomics
    in those sums it was 874 .. 1,304 parameters by one ulp)."""
    from paradis_model_amd.harness import rollout_loss
    batch = batches[0]
    model_u, _, _, step_u = _setup(optimizer=optimizer)
    step_u(batch)
    g_u = _grads(model_u)
    n64 = _norm64(g_u)
    assert n64 > 0
    # ---- clips
    model_c, _, _, step_c = _setup(optimizer=optimizer, gradient_clip_val=0.5 * n64)
    step_c(batch)
    norm, coef = step_c.last_grad_norm.clone()
    assert abs(float(norm) - n64) <= EPS23 * n64, (float(norm), n64)
    assert abs(float(coef) - 0.5 * n64 / (n64 + 1e-6)) <= EPS23 and float(coef) < 1.0
    covered = {id(p) for group in step_c.opt.param_groups for p in group["params"]}
    assert covered == {id(p) for p in model_c.parameters()}
    for p, g in zip(model_c.parameters(), g_u):
        assert (p.grad is None) == (g is None)
        if g is not None:
            assert torch.equal(p.grad, g * coef)
    # ---- the twin whose gradients are multiplied by that coefficient before its optimiser step
    model_m, loss_m, _, step_m = _setup(optimizer=optimizer)
    step_m.opt.zero_grad(set_to_none=True)
    rollout_loss(model_m, loss_m, batch, num_common=83, n_inputs=2)
    for p in model_m.parameters():
        if p.grad is not None:
            p.grad.mul_(coef)
    step_m.opt.step()
    # ---- does not clip
    model_l, _, _, step_l = _setup(optimizer=optimizer, gradient_clip_val=2.0 * n64)
    step_l(batch)
    assert float(step_l.last_grad_norm[1]) == 1.0
    for p, g in zip(model_l.parameters(), g_u):
        assert g is None or torch.equal(p.grad, g)
    pc, pm, pl, pu = _flat(model_c), _flat(model_m), _flat(model_l), _flat(model_u)
    print("MEASURED | clipping in the step, %s | clipped vs mul_ twin: %d of %d parameters differ, max_rel %.3e | "
          "not clipped vs unclipped twin: %d differ, max_rel %.3e"
          % (optimizer, int((pc != pm).sum()), pc.numel(), max_rel(pc, pm), int((pl != pu).sum()), max_rel(pl, pu)))
    assert not torch.equal(pc, pu)
    # the parameters that AdamW kernels update are bit-equal under either optimiser
    adamw = [i for i, group in enumerate(step_c.opt.param_groups) if group.get("algorithm", "adamw") == "adamw"]
    for i in adamw:
        for a, b in zip(step_c.opt.param_groups[i]["params"], step_m.opt.param_groups[i]["params"]):
            assert torch.equal(a, b)
    assert torch.equal(pc, pm)
    assert torch.equal(pl, pu)


# ================================================================================================ 5. statistics
def test_statistics_see_unclipped_gradients(batches):
    from paradis_model_amd.diagnostics import TrainStats
    model, loss_fn, cfg, step = _setup(stats=True, gradient_clip_val=1e-3)
    step(batches[0])
    norm, coef = step.last_grad_norm.tolist()
    assert coef < 1.0                                               # it clips: the clipped norm would be 1e-3
    total = step.stats.result()["grad/total"]
    assert abs(total - norm) <= 2.0 ** -22 * norm, (total, norm)
    from paradis_model_amd.harness import TrainStep
    with pytest.raises(ValueError, match="stats"):
        TrainStep(model, loss_fn, cfg, stats=TrainStats(model, loss_fn, channel_losses=False), accumulate_grad_batches=2)


# ================================================================================================ 6. truncated BPTT
def _tbptt_figures():
    from paradis_model_amd.harness import assemble_model_input, next_input, rollout_loss
    batch = _batches(1, S=3)[0]
    inp, tgt, forc, const = batch
    # what TrainStep leaves with detach_gradient_every = 1, and with full BPTT
    model_t, _, _, step_t = _setup(detach=1)
    assert step_t.detach_every == 1
    step_t(batch)
    g_trunc = _grads(model_t)
    model_f, _, _, step_f = _setup(detach=None)
    step_f(batch)
    g_full = _grads(model_f)
    # the expected gradients from public pieces: the inputs of a no-grad rollout, then three single-step calls
    model_x, loss_x, _, step_x = _setup()
    with torch.no_grad():
        _, outs = rollout_loss(model_x, loss_x, batch, num_common=83, n_inputs=2, backward=False, keep_outputs=True)
        inputs = [inp]
        constants = const[:, :1].permute(0, 1, 4, 2, 3)
        forcings = forc.permute(0, 1, 4, 2, 3)
        for s in range(2):
            mi = assemble_model_input(inputs[s], forcings[:, s].unsqueeze(1), constants)
            inputs.append(next_input(mi, outs[s], 83, 2).unsqueeze(1))
    step_x.opt.zero_grad(set_to_none=True)
    for s in range(3):
        single = (inputs[s], tgt[:, s:s + 1], forc[:, s:s + 1], const)
        rollout_loss(model_x, loss_x, single, num_common=83, n_inputs=2, accum=3)
    g_expect = _grads(model_x)
    torch.cuda.synchronize()
    return dict(trunc=_rel_per_tensor(g_trunc, g_expect), full=_rel_per_tensor(g_full, g_trunc))


def test_detach_gradient_every_one_truncates_the_backward():
    r = _tbptt_figures()
    print("MEASURED | detach_gradient_every=1, S=3 | against three single-step calls %.3e | full BPTT against truncated %.3e"
          % (r["trunc"], r["full"]))
    assert r["trunc"] <= TBPTT_GRAD_BOUND, r["trunc"]
    # a missing detach would leave the full-BPTT gradients: they must be far outside the bound
    assert r["full"] >= 100 * TBPTT_GRAD_BOUND and r["full"] > 1e-4, r["full"]


# ================================================================================================ 7. graphed
def _check_replay(tag, le, lg, step_e, step_g):
    le, lg = le.reshape(-1).tolist(), lg.reshape(-1).tolist()
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * abs(a), (tag, le, lg)
    if step_e.last_grad_norm is not None:
        ne, ng = step_e.last_grad_norm.tolist(), step_g.last_grad_norm.tolist()
        for a, b in zip(ne, ng):
            assert abs(a - b) <= 1e-6 * abs(a), (tag, ne, ng)


def test_graphed_window_with_clipping_equals_eager():
    from paradis_model_amd.harness import GraphedTrainStep
    bs = _batches(4)
    windows = [bs[0:2], bs[2:4]]
    small = [tuple(t[:1].contiguous() for t in b) for b in windows[1]]
    # the clip value: half the norm of the first window of an unclipped twin
    _, _, _, probe = _setup(accumulate_grad_batches=2, gradient_clip_val=1e30)
    probe.window(windows[0])
    norm0, coef0 = probe.last_grad_norm.tolist()
    assert coef0 == 1.0 and norm0 > 0
    clip_val = 0.5 * norm0
    model_e, _, _, step_e = _setup(accumulate_grad_batches=2, gradient_clip_val=clip_val)
    model_g, _, _, step_g = _setup(capturable=True, accumulate_grad_batches=2, gradient_clip_val=clip_val)
    with pytest.raises(ValueError, match="sequence of 2"):
        GraphedTrainStep(step_g, windows[0][0])
    warm = 2
    g = GraphedTrainStep(step_g, windows[0], warmup=warm)
    for i in range(warm):
        step_e.window(windows[0])
        if i == 0:
            assert float(step_e.last_grad_norm[1]) < 1.0           # the clip bites on the first window
    n_windows = warm
    for tag, (window, graphed) in enumerate(((windows[0], True), (windows[1], True), (small, False), (windows[1], True))):
        le = step_e.window(window)
        lg = g(window) if graphed else g.eager_step(window)
        assert lg.shape == (2,)
        _check_replay(tag, le, lg, step_e, step_g)
        n_windows += 1
    torch.cuda.synchronize()
    err = max_rel(_flat(model_g), _flat(model_e))
    print(f"MEASURED | graphed window N=2 with clipping | parameters {err:.3e}")
    assert err <= 1e-6, err
    assert step_g.pending == 0 and step_g.opt_steps == n_windows and step_e.opt_steps == n_windows
    st = step_g.opt.state[next(iter(model_g.parameters()))]
    assert int(st["step"]) == n_windows                            # one optimiser step per window, not per micro-batch


def test_graphed_truncated_bptt_equals_eager():
    from paradis_model_amd.harness import GraphedTrainStep
    bs = _batches(2, S=3)
    model_e, _, _, step_e = _setup(detach=2)
    model_g, _, _, step_g = _setup(capturable=True, detach=2)
    assert step_g.detach_every == 2
    warm = 2
    g = GraphedTrainStep(step_g, bs[0], warmup=warm)
    for _ in range(warm):
        step_e(bs[0])
    for i in (0, 1, 0):
        _check_replay(i, step_e(bs[i]), g(bs[i]), step_e, step_g)
    torch.cuda.synchronize()
    err = max_rel(_flat(model_g), _flat(model_e))
    print(f"MEASURED | graphed detach_gradient_every=2, S=3 | parameters {err:.3e}")
    assert err <= 1e-6, err
    # the truncation is in the captured step: full BPTT moves the parameters elsewhere
    model_f, _, _, step_f = _setup(detach=None)
    for i in (0, 0, 0, 1, 0):
        step_f(bs[i])
    assert max_rel(_flat(model_f), _flat(model_e)) > 1e-5
