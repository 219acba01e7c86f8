"""GPU: the training diagnostics - the statistics launch pair ``paradis_param_stats`` against plain fp64
(tests/stats_oracle.py) at its dispatch edges, ``diagnostics.TrainStats`` through real training steps (AdamW and
NorMuon), its neutrality (a step with statistics moves the parameters exactly as one without) and its HIP-graph form.

Protocol of the comparisons: that of tests/test_hip_kernel_edges.py.  Every compared number is a scalar; for sums, norms
and ratios e = |x - ref64| / |ref64|, for the alignments (cosines, in [-1, 1]) e = |x - ref64|.  e_hip is the kernel's,
e_cpu that of the oracle evaluated in fp32 in the reference's operation order - for groups of at least 256 elements the
larger of torch.sum's error and a strictly sequential fp32 accumulation's.  Asserted: e_hip <= 1e-5 (SURVEY.md 8c ii) and
e_hip <= 1.5 e_cpu + 1e-7 (8c iii).  Every figure is printed (``-s``) and recorded as a property.

Input design of test 1: the first and last element of every tensor and the element in front of every chunk boundary are
2^10 times the rest, in the parameter, the gradient and the moment; one case has strictly positive values, so nothing
cancels; the moments are 0.5 g + 0.3 noise (cosines ~0.86 with normal values, higher with positive ones)."""
import functools

import pytest
import torch

from paradis_model_amd.config import reduced_config, stub_datamodule
from tests import stats_oracle as SO
from tests._util import make_grid

pytestmark = pytest.mark.gpu
CEIL = 1e-5
SPIKE = 1024.0
COLS = ("sum p^2", "sum g^2", "sum g.m", "sum m^2", "grad", "gradratio", "pnorm", "alignment")


class _Judge:
    """collects e_hip / e_cpu per number, prints and records them, asserts both bounds at the end"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad = record_property, case, []

    def add(self, name, got, ref, cpu, seq=None, absolute=False):
        scale = 1.0 if absolute else max(abs(ref), 1e-300)
        e_hip, e_cpu = abs(got - ref) / scale, abs(cpu - ref) / scale
        if seq is not None:
            e_cpu = max(e_cpu, abs(seq - ref) / scale)
        print(f"STATS | {self.case} | {name} | e_hip {e_hip:.2e} | e_cpu {e_cpu:.2e}")
        self.rp(name, f"e_hip={e_hip:.3e} e_cpu={e_cpu:.3e}")
        if not e_hip <= CEIL:
            self.bad.append((name, "ceiling", e_hip, CEIL))
        if not e_hip <= 1.5 * e_cpu + 1e-7:
            self.bad.append((name, "fp32 yardstick", e_hip, e_cpu))

    def done(self):
        assert not self.bad, (self.case, self.bad)


def _judge_logged(J, got, named, grads, moments, tag=""):
    """a dict of logged values against the oracle fed with CPU tensors; the key sets must agree"""
    r64, _ = SO.metrics(named, grads, moments)
    r32, _ = SO.metrics(named, grads, moments, torch.float32)
    rseq, _ = SO.metrics(named, grads, moments, torch.float32, seq=True)
    assert set(got) == set(r64), (sorted(set(got) ^ set(r64)))
    size = {}
    for (name, p) in named:
        size[name.split(".")[1]] = size.get(name.split(".")[1], 0) + p.numel()
    size["total"] = sum(size.values())
    for k in sorted(r64):
        big = size[k.split("/")[1]] >= 256
        J.add(tag + k, got[k], r64[k], r32[k], rseq[k] if big else None, absolute=k.startswith("grad_alignment/"))
    return r64


# ================================================================================================ 1. the kernel pair
def _edge_spec(C):
    """(group key, numel, has gradient, has moment); the chunk size C is where the kernel starts another workgroup"""
    return [("edges", 1, True, True), ("edges", 3, True, True), ("edges", C - 1, True, True), ("edges", C, True, True),
            ("edges", C + 1, True, True), ("edges", 2 * C + 5, True, True),
            ("mixed", C + 7, True, True),            # in the offset run: a view one float into its storage
            ("mixed", 1030, False, True),            # no gradient: its moment must not be read
            ("mixed", 2 * C - 3, True, False),       # a gradient but no moment: counts in sum g^2 only
            ("single", 1000, True, True),            # a group holding one tensor
            ("nograd", 5, False, False), ("nograd", C + 3, False, True),      # a group without any gradient
            ("nomoment", 777, True, False), ("nomoment", 4, True, False)]     # gradients, no moment at all


@functools.lru_cache(maxsize=None)
def _edge_inputs(C, positive):
    """CPU tensors (named, grads, moments); the references are formed from them: built once per case"""
    g = torch.Generator().manual_seed(31 + int(positive))
    named, grads, moments = [], [], []

    def draw(n):
        return (torch.rand(n, generator=g) + 0.5) if positive else torch.randn(n, generator=g)

    for i, (key, n, has_g, has_m) in enumerate(_edge_spec(C)):
        pos = sorted({0, n - 1} | {k * C - 1 for k in range(1, (n + C - 1) // C + 1) if k * C - 1 < n})
        p, gr = draw(n), draw(n) * 0.01
        p[pos] *= SPIKE
        gr[pos] *= SPIKE
        m = 0.5 * gr + 0.3 * 0.01 * draw(n)
        named.append((f"model.{key}.t{i}", p))
        grads.append(gr if has_g else None)
        moments.append(m if has_m else None)
    return named, grads, moments


def _to_device(ts, offset):
    """dense device copies; ``offset``: every tensor is a view starting 4 bytes past a 16-byte boundary"""
    out = []
    for t in ts:
        if t is None:
            out.append(None)
        elif offset:
            buf = torch.zeros(t.numel() + 1, device="cuda")
            assert buf.data_ptr() % 16 == 0
            v = buf[1:].copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            out.append(v)
        else:
            v = t.cuda()
            assert v.data_ptr() % 16 == 0
            out.append(v)
    return out


@pytest.mark.parametrize("positive", [False, True], ids=["normal", "positive"])
def test_param_stats_kernel_at_dispatch_edges(record_property, positive):
    from paradis_model_amd import _lib
    from paradis_model_amd.diagnostics import StatsPlan, param_stats
    C = _lib.lib.paradis_param_stats_chunk()
    named, grads, moments = _edge_inputs(C, positive)
    keys = sorted({n.split(".")[1] for n, _ in named})
    groups = [keys.index(n.split(".")[1]) for n, _ in named]
    G = len(keys)

    def run(offset, mixed_alignment=False):
        ps = _to_device([p for _, p in named], offset)
        gs = _to_device(grads, offset and not mixed_alignment)
        ms = _to_device(moments, offset)
        plan = StatsPlan([p.numel() for p in ps], groups, G, "cuda")
        plan.out.fill_(float("nan"))
        first = param_stats(ps, gs, ms, groups, plan=plan).clone()
        plan.out.fill_(float("nan"))
        assert torch.equal(param_stats(ps, gs, ms, groups, plan=plan), first)      # two launches: the same bits
        for (_, p), d in zip(named, ps):
            assert torch.equal(d.cpu(), p)                                             # the inputs are not written
        return first

    got_d = run(False)
    assert torch.equal(run(True), got_d)                  # the scalar path on the same data: the same bits
    assert torch.equal(run(True, mixed_alignment=True), got_d)      # one tensor of a chunk misaligned: scalar for all three
    assert torch.equal(param_stats(_to_device([p for _, p in named], False), _to_device(grads, False),
                                   _to_device(moments, False), groups), got_d)   # without a plan, G from the indices
    got = got_d.cpu().double()
    assert got.shape == (G + 1, 8) and bool(torch.isfinite(got).all())

    _, s64 = SO.metrics(named, grads, moments)
    _, s32 = SO.metrics(named, grads, moments, torch.float32)
    _, sseq = SO.metrics(named, grads, moments, torch.float32, seq=True)
    J = _Judge(record_property, f"param_stats {'positive' if positive else 'normal'}")

    def derived(s):
        p2, g2, gm, m2 = s
        pn = max(p2 ** 0.5, 1e-12)
        return list(s) + [g2 ** 0.5, g2 ** 0.5 / pn, pn, gm / (g2 ** 0.5 * m2 ** 0.5 + 1e-12) if m2 > 0 else 0.0]

    size = {k: sum(p.numel() for n, p in named if n.split(".")[1] == k) for k in keys}
    size["total"] = sum(size.values())
    for row, k in enumerate(keys + ["total"]):
        r, c, q = derived(s64[k]), derived(s32[k]), derived(sseq[k])
        for j, col in enumerate(COLS):
            if r[j] == 0.0:
                assert float(got[row, j]) == 0.0, (k, col)           # nothing to sum: exactly zero
                continue
            J.add(f"{k} {col}", float(got[row, j]), r[j], c[j], q[j] if size[k] >= 256 else None, absolute=(j == 7))
    # what is absent stays out: the group without gradients has only its parameter norm, the moments of tensors
    # without a gradient are not read, a group without moments has no alignment
    ng, nm = keys.index("nograd"), keys.index("nomoment")
    assert got[ng, 1:6].abs().max() == 0 and got[ng, 7] == 0 and got[ng, 0] > 0 and got[ng, 6] > 0
    assert got[nm, 1] > 0 and got[nm, 2] == 0 and got[nm, 3] == 0 and got[nm, 7] == 0
    assert 0.3 < float(got[keys.index("edges"), 7]) <= 1.0
    J.done()


def test_param_stats_without_chunks_and_non_contiguous():
    from paradis_model_amd.diagnostics import StatsPlan, param_stats
    plan = StatsPlan([0], [1], 2, "cuda")                 # one empty tensor: no chunk at all, the finish kernel still runs
    plan.out.fill_(float("nan"))
    e = torch.zeros(0, device="cuda")
    out = param_stats([e], [e], [e], [1], plan=plan).cpu()
    assert plan.n_chunks == 0
    want = torch.zeros(3, 8)
    want[:, 6] = 1e-12
    assert torch.equal(out, want)
    w = torch.randn(8, 6, device="cuda")
    with pytest.raises(RuntimeError, match="non-contiguous"):
        param_stats([w.t()], [None], [None], [0])
    with pytest.raises(RuntimeError, match="non-contiguous"):
        param_stats([w], [w.t()], [None], [0])
    with pytest.raises(RuntimeError, match="non-contiguous"):
        param_stats([w], [w], [w.t()], [0])
    with pytest.raises(RuntimeError, match="fp32"):
        param_stats([w], [w.double()], [None], [0])


# ================================================================================================ 2. through the step
def _setup(nlat=16, nlon=32, optimizer="adamw", capturable=False, stats=True, channel_losses=True):
    from paradis_model_amd.diagnostics import TrainStats
    from paradis_model_amd.harness import TrainStep
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = reduced_config()
    cfg.training.optimizer.name = optimizer
    lat_deg, lg, og = make_grid(nlat, nlon, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda()
    loss = build_loss(cfg, lat_deg).cuda()
    ts = TrainStats(model, loss, channel_losses=channel_losses) if stats else None
    return model, loss, TrainStep(model, loss, cfg, capturable=capturable, stats=ts), ts, (cfg, lat_deg)


def _manual_step(step, batch):
    """``TrainStep.__call__`` with the statistics, stopped in front of ``before_optimizer_step`` to copy what it will read"""
    from paradis_model_amd.harness import rollout_loss
    ts = step.stats
    step.opt.zero_grad(set_to_none=True)
    ts.begin_step()
    loss, outs = rollout_loss(step.model, step.loss_fn, batch, num_common=step.num_common, n_inputs=step.n_inputs,
                              detach_every=step.detach_every, keep_outputs=True, on_step=ts.on_rollout_step)
    named, grads, moments = [], [], []
    for name, p in step.model.named_parameters():
        named.append(("model." + name, p.detach().cpu().clone()))
        grads.append(None if p.grad is None else p.grad.detach().cpu().clone())
        st = step.opt.state.get(p)
        moments.append(st["exp_avg"].detach().cpu().clone() if st and "exp_avg" in st and p.grad is not None else None)
    ts.before_optimizer_step(step.opt)
    ts.record_loss(loss)
    step.opt.step()
    return loss, [o.cpu() for o in outs], named, grads, moments


def _split(res):
    grad = {k: v for k, v in res.items() if not k.startswith("train_loss")}
    return grad, {k: v for k, v in res.items() if k.startswith("train_loss")}


def test_trainstats_through_two_adamw_steps(record_property):
    from paradis_model_amd.harness import synthetic_batch
    from paradis_model_amd.loss import build_loss
    from tests import val_oracle as VO
    from tests.test_stats_cpu import REFERENCE_KEYS
    model, loss_fn, step, ts, (cfg, lat_deg) = _setup()
    cpu32 = build_loss(cfg, lat_deg)
    cpu64 = build_loss(cfg, lat_deg).double()
    names = list(loss_fn.output_name_order)
    C = len(names)
    J = _Judge(record_property, "TrainStats adamw")
    for it in range(2):
        batch = synthetic_batch(16, 32, False, 2, 2, seed=5 + it, device="cuda")
        loss, outs, named, grads, moments = _manual_step(step, batch)
        res = ts.result()
        got, train = _split(res)
        r64 = _judge_logged(J, got, named, grads, moments, tag=f"step {it + 1} ")
        align = {k for k in got if k.startswith("grad_alignment/")}
        if it == 0:
            assert not align                                          # no optimiser state yet
        else:
            assert align == {f"grad_alignment/{k}" for k in REFERENCE_KEYS + ["total"]}
            assert all(-1.0 <= got[k] <= 1.0 for k in align)
        assert {k.split("/")[1] for k in r64} == set(REFERENCE_KEYS + ["total"])
        # the losses
        assert set(train) == {"train_loss"} | {f"train_loss_channel_{w}/{n}" for w in ("weighted", "unweighted") for n in names}
        assert train["train_loss"] == float(loss)
        tgt = batch[1].cpu()
        wf, lat = cpu32.feature_weights.float(), cpu32.lat_weights.float()
        wl = lat if cpu32.apply_latitude_weights else None
        for weighted, off in ((True, 1), (False, 1 + C)):
            tag = "weighted" if weighted else "unweighted"
            ref = sum(cpu64.per_channel_loss(o.double(), tgt[:, s].double(), weighted=weighted) for s, o in enumerate(outs)) / len(outs)
            cpu = sum(cpu32.per_channel_loss(o, tgt[:, s], weighted=weighted).float() for s, o in enumerate(outs)) / len(outs)
            seq = sum(VO.row(o, tgt[:, s], wf, wl, lat, cpu32.kind, float(cpu32.delta), [], dtype=torch.float32,
                             seq=True)[off:off + C] for s, o in enumerate(outs)) / len(outs)
            mine = torch.tensor([train[f"train_loss_channel_{tag}/{n}"] for n in names], dtype=torch.float64)
            scale = float(ref.abs().max())
            e_hip = float((mine - ref).abs().max()) / scale
            e_cpu = max(float((cpu.double() - ref).abs().max()), float((seq.double() - ref).abs().max())) / scale
            print(f"STATS | step {it + 1} | per-channel {tag} | e_hip {e_hip:.2e} | e_cpu {e_cpu:.2e}")
            record_property(f"step {it + 1} per-channel {tag}", f"e_hip={e_hip:.3e} e_cpu={e_cpu:.3e}")
            assert e_hip <= CEIL and e_hip <= 1.5 * e_cpu + 1e-7, (tag, e_hip, e_cpu)
    J.done()


def test_trainstats_normuon_aligns_only_the_adamw_parameters(record_property):
    from paradis_model_amd.harness import synthetic_batch
    model, loss_fn, step, ts, _ = _setup(optimizer="normuon", channel_losses=False)
    J = _Judge(record_property, "TrainStats normuon")
    for it in range(2):
        batch = synthetic_batch(16, 32, False, 2, 2, seed=5 + it, device="cuda")
        _, _, named, grads, moments = _manual_step(step, batch)
    # the matrices keep "momentum", not "exp_avg": they were handed to the oracle without a moment
    matrix = {id(p) for g in step.opt.param_groups if g["algorithm"] != "adamw" for p in g["params"]}
    params = list(model.parameters())
    assert matrix and len(matrix) < len(params)
    for p, m in zip(params, moments):
        assert (m is None) == (id(p) in matrix)
        if id(p) in matrix:
            assert "momentum" in step.opt.state[p] and "exp_avg" not in step.opt.state[p]
    got, train = _split(ts.result())
    assert set(train) == {"train_loss"}                               # channel_losses=False
    _judge_logged(J, got, named, grads, moments)
    with_adamw = {n.split(".")[1] for (n, _), m in zip(named, moments) if m is not None}
    assert {k.split("/")[1] for k in got if k.startswith("grad_alignment/")} == with_adamw | {"total"}
    J.done()


# ================================================================================================ 3. no disturbance
def test_statistics_do_not_disturb_the_step():
    """three steps with and without the statistics from one initialisation and the same batches: bit-identical losses
    and parameters (the 32x64 step is bit-reproducible)"""
    from paradis_model_amd.harness import synthetic_batch
    batches = [synthetic_batch(32, 64, False, 2, 2, seed=5 + i, device="cuda") for i in range(3)]
    runs = []
    for stats in (True, False):
        model, _, step, ts, _ = _setup(32, 64, stats=stats)
        losses = [step(b).clone() for b in batches]
        if stats:
            res = ts.result()
            assert res["train_loss"] == float(losses[-1]) and res["grad/total"] > 0
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in model.parameters()]))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


# ================================================================================================ 4. HIP graph
def _close(a, b):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k in a:
        tol = 1e-6 if k.startswith("grad_alignment/") else 1e-6 * abs(b[k])
        assert abs(a[k] - b[k]) <= tol, (k, a[k], b[k])


def test_graphed_step_with_statistics_equals_eager_twin():
    from paradis_model_amd.harness import GraphedTrainStep, synthetic_batch
    batches = [synthetic_batch(16, 32, False, 2, 2, seed=5 + i, device="cuda") for i in range(2)]
    small = tuple(t[:1].contiguous() for t in batches[1])
    _, _, step_e, ts_e, _ = _setup()
    _, _, step_g, ts_g, _ = _setup(capturable=True)
    warm = 2
    g = GraphedTrainStep(step_g, batches[0], warmup=warm)
    for _ in range(warm):
        step_e(batches[0])
    seen = []
    for i in range(3):
        step_e(batches[i % 2])
        g(batches[i % 2])
        re_, rg = ts_e.result(), ts_g.result()
        _close(rg, re_)
        assert "grad_alignment/total" in rg and len(rg) == 2 + 4 * 8 + 2 * 97 + 1
        seen.append(rg)
    assert seen[1]["grad/total"] != seen[0]["grad/total"]             # result() follows the replays
    # an eager step on another batch rewrites the pinned address table; the next replay still reads its own tensors
    step_e(small)
    g.eager_step(small)
    _close(ts_g.result(), ts_e.result())
    step_e(batches[0])
    g(batches[0])
    _close(ts_g.result(), ts_e.result())
    torch.cuda.synchronize()
