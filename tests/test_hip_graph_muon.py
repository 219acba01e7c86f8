"""GPU: Muon / NorMuon steps inside the captured training step (harness.GraphedTrainStep) and learning-rate schedules that
run on the device (paradis_model_amd/schedule.py).  Set-up of tests/test_hip_graph.py: reduced model (tall, wide and
depthwise-conv matrices: both Newton-Schulz orientations and ``flatten``), 16x32 without poles, B = 2, S = 2, two
alternating batches.  Twins are eager, non-capturable ``TrainStep(schedule=...)`` runs over the same batch order."""
import struct

import numpy as np
import pytest
import torch

from paradis_model_amd.config import reduced_config, stub_datamodule
from tests._util import make_grid, max_rel

pytestmark = pytest.mark.gpu

# Final parameters, graphed against eager (max_rel): 1e-6, the bound of the AdamW graph test - unless two IDENTICAL eager
# NorMuon runs already differ by more than 3e-7 (the norm sums of the Muon step use float atomics), in which case the
# bound is 3 x that spread (two independent runs plus the <= 1 ulp difference of the device-side coefficients).
# MEASURED (MI355X, 10 steps of this set-up under the schedule below, the library of the commit before this feature, three
# runs per optimiser): NorMuon 1.2e-7 .. 2.4e-7 (losses 0 .. 7.9e-8), Muon 1.2e-7 .. 2.4e-7, AdamW 0 (bit-reproducible).
EAGER_SPREAD = 2.35e-7
PARAM_BOUND = 1e-6 if EAGER_SPREAD <= 3e-7 else 3 * EAGER_SPREAD

TOTAL, WARMUP, DECAY = 9, 4, 3          # k = 0..3 warm-up, 4..6 steady, 7..8 decay; k >= 9: the last entry holds


def _wsd():
    from paradis_model_amd.schedule import wsd_lambda
    return wsd_lambda(TOTAL, WARMUP, DECAY), TOTAL


def _setup(optimizer, capturable, schedule=None, stats=False, weight_decay=None):
    from paradis_model_amd.diagnostics import TrainStats
    from paradis_model_amd.harness import TrainStep
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = reduced_config()
    cfg.training.optimizer.name = optimizer
    if weight_decay is not None:
        cfg.training.optimizer.weight_decay = weight_decay
    lat_deg, lg, og = make_grid(16, 32, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda()
    loss = build_loss(cfg, lat_deg).cuda()
    ts = TrainStats(model, loss, channel_losses=False) if stats else None
    return model, TrainStep(model, loss, cfg, capturable=capturable, schedule=schedule, stats=ts)


@pytest.fixture(scope="module")
def batches():
    from paradis_model_amd.harness import synthetic_batch
    return [synthetic_batch(16, 32, False, 2, 2, seed=5 + i, device="cuda") for i in range(2)]


def _flat(model):
    return torch.cat([p.detach().flatten() for p in model.parameters()])


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


# ================================================================================================ 1. the kernel
N_TWINS = 6


@pytest.mark.parametrize("cls_name,nesterov", [("Muon", False), ("Muon", True), ("NorMuon", False)])
@pytest.mark.parametrize("split", [True, False])
def test_device_lr_equals_host_lr(cls_name, nesterov, split, monkeypatch):
    """One step of ``paradis_muon_step_d`` with the learning rate in a device state against ``paradis_muon_step`` with the
    same fp32 learning rate as a host scalar, on cloned inputs.  Per matrix: max|dw| <= 1e-6 max|update| + twin spread,
    the twin spread being the difference between identical calls of the host-scalar entry.

    When this test was written the norm sums of the step used float atomics, and identical calls landed on one of a few
    outcomes one ulp of ``w`` apart; the twin spread allowed for that.  The sums are now reduced in a fixed order
    (muon.hip, block_sum_fixed: per-workgroup partials added the same way by every consumer), so identical calls give
    identical bits - tests/test_hip_muon_edges.py::test_two_identical_steps_give_identical_bits holds the kernel to
    it - and the twin spread is expected to be 0.  The procedure is kept as it was: each entry is called N_TWINS times,
    the twin spread is the largest difference among the host calls, the device-vs-host difference the smallest over
    all pairs of a device and a host call - a systematic error of the device-side coefficients is in every such pair,
    and 1e-6 max|update| stays the bound on it.  A device learning rate of 0 leaves the weights bit-unchanged whatever
    the weight decay."""
    from paradis_model_amd import _lib, ops, optim
    monkeypatch.setattr(ops, "GEMM_SCHEME", ops.GEMM_BF16X3 if split else ops.GEMM_EXACT)
    calls = {"muon_step": 0, "muon_step_d": 0}

    class _Counting:
        def __getattr__(self, name):
            fn = getattr(_lib.lib, name)
            if name[8:] in calls:
                calls[name[8:]] += 1
            return fn
    monkeypatch.setattr(optim, "lib", _Counting())
    torch.manual_seed(1)
    shapes = [(64, 48), (48, 64), (64, 48), (32, 16, 1, 1), (40, 1, 3, 3), (20, 8), (130, 258)]
    w0 = [torch.randn(*s) * 0.1 for s in shapes]
    g0 = [torch.randn(*s) * 0.5 for s in shapes]
    lr = float(np.float32(5e-3))
    cls = getattr(optim, cls_name)

    def one_step(capturable, lr):
        ps = [torch.nn.Parameter(w.clone().cuda()) for w in w0]
        opt = cls([dict(params=ps, algorithm=cls_name.lower(), flatten=True)], lr=lr, weight_decay=1e-2,
                  betas=(0.9, 0.95), nesterov=nesterov, capturable=capturable)
        for p, g in zip(ps, g0):
            p.grad = g.clone().cuda()
        opt.step()
        torch.cuda.synchronize()
        return opt, [p.detach().cpu() for p in ps]

    host = [one_step(False, lr)[1] for _ in range(N_TWINS)]
    assert calls == {"muon_step": 6 * N_TWINS, "muon_step_d": 0}            # six distinct shapes per step
    device = []
    for _ in range(N_TWINS):
        opt_d, w = one_step(True, lr)
        assert opt_d._dev_state[0][0].tolist() == [1, _bits(lr)]           # ticked once, the rate as the device holds it
        device.append(w)
    assert calls == {"muon_step": 6 * N_TWINS, "muon_step_d": 6 * N_TWINS}
    for i, s in enumerate(shapes):
        upd = float((host[0][i] - w0[i]).abs().max())
        spread = max(float((a[i] - b[i]).abs().max()) for a in host for b in host)
        err = min(float((d[i] - h[i]).abs().max()) for d in device for h in host)
        print(f"MEASURED | {cls_name} nesterov={nesterov} split={split} {s} | device-vs-host {err:.3e} | "
              f"twin spread {spread:.3e} | update {upd:.3e}")
        assert upd > 1e-4
        assert err <= 1e-6 * upd + spread, (cls_name, s, err, upd, spread)
    _, frozen = one_step(True, 0.0)
    for i in range(len(shapes)):
        assert torch.equal(frozen[i], w0[i])


# ================================================================================================ 2. graphed = eager
@pytest.mark.parametrize("optimizer", ["normuon", "muon", "adamw"])
def test_graphed_equals_eager_under_wsd(optimizer, batches):
    """2 eager warm-up steps + 8 replays under the warm-up / steady / decay schedule (two replays still in the warm-up,
    three steady, two decaying, one past the end of the table) against 10 eager steps with the same learning rates set
    on the host.  Losses to 1e-6 relative, final parameters to PARAM_BOUND.

    MEASURED (MI355X): eager-vs-eager spread of identical NorMuon runs 2.35e-7 at most (EAGER_SPREAD, not above 3e-7), so
    the bound used is 1e-6 (PARAM_BOUND); graphed against eager: NorMuon 1.2e-7 (losses 7.9e-8), Muon 1.2e-7, AdamW 0."""
    from paradis_model_amd.harness import GraphedTrainStep
    warm, n_replays = 2, 8
    order = [0] * warm + [i % 2 for i in range(n_replays)]
    model_e, step_e = _setup(optimizer, False, schedule=_wsd())
    losses_e, lrs_e = [], []
    for i in order:
        losses_e.append(float(step_e(batches[i])))
        lrs_e.append([g["lr"] for g in step_e.opt.param_groups])
    model_g, step_g = _setup(optimizer, True, schedule=_wsd())
    g = GraphedTrainStep(step_g, batches[0], warmup=warm)
    sched = step_g.opt._schedule
    losses_g, lrs_g = [], []
    for i in order[warm:]:
        losses_g.append(float(g(batches[i])))
        lrs_g.append([grp["lr"] for grp in step_g.opt.param_groups])
    torch.cuda.synchronize()
    n_steps = warm + n_replays
    assert lrs_g == lrs_e[warm:]                                   # the host mirror follows the replays
    base = step_e.schedule.base_lrs[0]
    assert [l[0] for l in lrs_e] == [float(np.float32(base * m)) for m in
                                     (.25, .5, .75, 1, 1, 1, 1, 2 / 3, 1 / 3, 1 / 3)]
    for gi, grp in enumerate(step_g.opt.param_groups):
        assert grp["lr"] == sched.host_lr(gi, n_steps - 1)
        # ... and it is what the device holds: step count and the bits of the rate
        assert step_g.opt._dev_state[gi][0].tolist() == [n_steps, _bits(sched.host_lr(gi, n_steps - 1))]
    rel = [abs(a - b) / abs(a) for a, b in zip(losses_e[warm:], losses_g)]
    err = max_rel(_flat(model_g), _flat(model_e))
    print(f"MEASURED | {optimizer} | graphed-vs-eager parameters {err:.3e} | losses {max(rel):.3e}")
    for p in model_g.parameters():
        assert int(step_g.opt.state[p]["step"]) == n_steps
    assert max(rel) <= 1e-6, (losses_e, losses_g)
    assert err <= PARAM_BOUND, err


# ================================================================================================ 3. inside the graph
def test_schedule_acts_inside_the_graph(batches):
    """a table that is zero from its fifth entry on: the replays of steps 3 and 4 move the parameters, those of steps
    5, 6 and 7 (the last one past the end of the table) leave every parameter bit-unchanged (weight_decay = 0)"""
    from paradis_model_amd.harness import GraphedTrainStep
    model, step = _setup("normuon", True, schedule=(lambda k: 1.0 if k < 4 else 0.0, 6), weight_decay=0.0)
    g = GraphedTrainStep(step, batches[0], warmup=2)
    matrix = [p for grp in step.opt.param_groups if grp["algorithm"] != "adamw" for p in grp["params"]]
    assert matrix
    snaps = [[p.detach().clone() for p in matrix]]
    flats = [_flat(model).clone()]
    for i in range(5):
        g(batches[i % 2])
        torch.cuda.synchronize()
        snaps.append([p.detach().clone() for p in matrix])
        flats.append(_flat(model).clone())
    for a, b in ((0, 1), (1, 2)):
        assert all(not torch.equal(x, y) for x, y in zip(snaps[a], snaps[b]))
        assert max_rel(flats[b], flats[a]) > 1e-5
    for a, b in ((2, 3), (3, 4), (4, 5)):
        assert all(torch.equal(x, y) for x, y in zip(snaps[a], snaps[b]))
        assert torch.equal(flats[a], flats[b])                      # the AdamW group stands still too
    assert [grp["lr"] for grp in step.opt.param_groups] == [0.0, 0.0]


# ================================================================================================ 4. the host route
def test_host_route_reaches_the_right_group(batches):
    """NorMuon, the matrix group at 5e-4 and the AdamW group at 2e-4; between two replays only the AdamW group's rate
    changes (a host-side scheduler), followed by ``sync_device_state()``.  The next replay moves the matrices like the
    twin whose rates never changed and the other parameters like the twin whose AdamW rate changed."""
    from paradis_model_amd.harness import GraphedTrainStep
    warm = 2
    order = [0] * warm + [0, 1, 0]

    def lrs(step, adamw_lr):
        for grp in step.opt.param_groups:
            if grp["algorithm"] == "adamw":
                grp["lr"] = adamw_lr

    def split(model, step):
        matrix = {id(p) for grp in step.opt.param_groups if grp["algorithm"] != "adamw" for p in grp["params"]}
        ps = list(model.parameters())
        return (torch.cat([p.detach().flatten() for p in ps if id(p) in matrix]),
                torch.cat([p.detach().flatten() for p in ps if id(p) not in matrix]))

    twins = {}
    for name, late in (("unchanged", 2e-4), ("changed", 1e-3)):
        model, step = _setup("normuon", False)
        lrs(step, 2e-4)
        for n, i in enumerate(order):
            if n == len(order) - 1:
                lrs(step, late)
            step(batches[i])
        twins[name] = split(model, step)
    model_g, step_g = _setup("normuon", True)
    lrs(step_g, 2e-4)
    g = GraphedTrainStep(step_g, batches[0], warmup=warm)
    for i in order[warm:-1]:
        g(batches[i])
    lrs(step_g, 1e-3)
    step_g.opt.sync_device_state()
    g(batches[order[-1]])
    torch.cuda.synchronize()
    mat, rest = split(model_g, step_g)
    e_mat, e_rest = max_rel(mat, twins["unchanged"][0]), max_rel(rest, twins["changed"][1])
    moved = max_rel(twins["changed"][1], twins["unchanged"][1])
    print(f"MEASURED | host route | matrices {e_mat:.3e} | AdamW parameters {e_rest:.3e} | the change itself {moved:.3e}")
    assert moved > 1e-4                                             # the two twins are told apart by far
    assert e_mat <= PARAM_BOUND and e_rest <= PARAM_BOUND
    states = step_g.opt._dev_state
    assert [_bits(grp["lr"]) for grp in step_g.opt.param_groups] == [states[0][0][1].item(), states[1][0][1].item()]


# ================================================================================================ 5. eager_step
def test_eager_step_between_replays_with_normuon(batches):
    """graph, eager on a B = 1 batch (which rewrites the pinned address tables of the matrix group and of the AdamW group),
    graph, graph - under the schedule, against the eager twin"""
    from paradis_model_amd.harness import GraphedTrainStep
    model_e, step_e = _setup("normuon", False, schedule=_wsd())
    model_g, step_g = _setup("normuon", True, schedule=_wsd())
    warm = 2
    g = GraphedTrainStep(step_g, batches[0], warmup=warm)
    assert {k[0] for k in g._tables} == {"_fused_cache", "_muon_cache"}
    for _ in range(warm):
        step_e(batches[0])
    small = tuple(t[:1].contiguous() for t in batches[1])
    for batch, graphed in ((batches[0], True), (small, False), (batches[1], True), (batches[0], True)):
        le = float(step_e(batch))
        lg = float(g(batch) if graphed else g.eager_step(batch))
        assert abs(le - lg) <= 1e-6 * abs(le), (le, lg, graphed)
        assert [grp["lr"] for grp in step_g.opt.param_groups] == [grp["lr"] for grp in step_e.opt.param_groups]
    torch.cuda.synchronize()
    err = max_rel(_flat(model_g), _flat(model_e))
    print(f"MEASURED | eager_step between replays | parameters {err:.3e}")
    assert err <= PARAM_BOUND, err
    assert all(int(step_g.opt.state[p]["step"]) == warm + 4 for p in model_g.parameters())


# ================================================================================================ 6. TrainStats
def test_trainstats_under_a_graphed_normuon_step(batches):
    """``stats.result()`` after a replay agrees with the eager twin's to 1e-6 (1e-6 absolute for the cosines); alignment
    keys appear only for groups that hold parameters of the AdamW group.

    The 1e-6 is asserted for the FIRST replay behind ONE warm-up step, i.e. at optimiser step 2.  Two identical eager
    NorMuon runs are bit-equal only at step 1: the float atomics of the Muon norm sums make them drift apart, and the
    smallest logged norm (grad/velocity_nets, 4e-5) amplifies that.  MEASURED eager-vs-eager on the commit before this
    feature, worst logged value of three runs: step 1: 0; step 2: 2.0e-7 .. 4.0e-7; step 3: 1.2e-6 .. 2.5e-6; step 4:
    2.3e-6 .. 2.0e-5; step 5: 4.1e-7 .. 5.0e-6 - so from step 3 on no implementation meets 1e-6 against a twin run (a
    first version of this test compared three replays behind two warm-up steps and missed by 9.2e-6 on
    grad/velocity_nets).  The later replays check the keys, that the values follow the replays, and print the distance."""
    from paradis_model_amd.diagnostics import group_key
    from paradis_model_amd.harness import GraphedTrainStep
    model_e, step_e = _setup("normuon", False, stats=True)
    model_g, step_g = _setup("normuon", True, stats=True)
    warm = 1
    g = GraphedTrainStep(step_g, batches[0], warmup=warm)
    for _ in range(warm):
        step_e(batches[0])
    matrix = {id(p) for grp in step_g.opt.param_groups if grp["algorithm"] != "adamw" for p in grp["params"]}
    with_adamw = {group_key(n) for n, p in model_g.named_parameters() if id(p) not in matrix}
    all_keys = {group_key(n) for n, _ in model_g.named_parameters()}
    assert with_adamw and matrix
    seen = []
    for i in range(3):
        step_e(batches[i % 2])
        g(batches[i % 2])
        re_, rg = step_e.stats.result(), step_g.stats.result()
        assert set(rg) == set(re_), sorted(set(rg) ^ set(re_))
        worst = max((abs(rg[k] - re_[k]) / (1.0 if k.startswith("grad_alignment/") else abs(re_[k])), k) for k in rg)
        print(f"MEASURED | statistics, replay {i + 1} (step {warm + i + 1}) | worst {worst[0]:.3e} at {worst[1]}")
        if i == 0:
            for k in rg:
                tol = 1e-6 if k.startswith("grad_alignment/") else 1e-6 * abs(re_[k])
                assert abs(rg[k] - re_[k]) <= tol, (k, rg[k], re_[k])
        assert {k.split("/")[1] for k in rg if k.startswith("grad_alignment/")} == with_adamw | {"total"}
        assert {k.split("/")[1] for k in rg if k.startswith("pnorm/")} == all_keys
        assert rg["train_loss"] == float(g.static_loss)
        seen.append(rg)
    assert seen[1]["grad/total"] != seen[0]["grad/total"]             # result() follows the replays
    torch.cuda.synchronize()


# ================================================================================================ 7. host time
def test_graphed_normuon_step_host_time_is_one_launch(batches):
    """what the graph buys: the host returns from a replay long before an eager NorMuon step has been enqueued"""
    import time
    from paradis_model_amd.harness import GraphedTrainStep
    model_e, step_e = _setup("normuon", False, schedule=_wsd())
    for _ in range(3):
        step_e(batches[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        step_e(batches[0])
    t_eager = (time.perf_counter() - t0) / 5          # host time to enqueue (no sync inside)
    torch.cuda.synchronize()
    model_g, step_g = _setup("normuon", True, schedule=_wsd())
    g = GraphedTrainStep(step_g, batches[0], warmup=2)
    g(batches[0]); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        g(batches[0])
    t_graph = (time.perf_counter() - t0) / 5
    torch.cuda.synchronize()
    print("MEASURED | host time per NorMuon step: eager %.2f ms, graph replay %.2f ms" % (1e3 * t_eager, 1e3 * t_graph))
    assert t_graph < 0.5 * t_eager
