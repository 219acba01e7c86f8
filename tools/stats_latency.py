"""Latency of the training diagnostics on the MI355X.

(a) The gradient statistics of the default model's 335 tensors (60 M parameters; parameters as initialised, gradients and
first moments seeded - no forward runs): the reference's ``on_before_optimizer_step`` loop restated on device tensors
(ATen calls per parameter: squares, products, full reductions, scalar adds, then the per-group norms and cosines) against
``diagnostics.param_stats`` with a cached plan.  For each: the host time to enqueue one call (nothing waits for the
device inside) and the device time per call (HIP events around ``iters`` calls), the two alternated in one process.
(b) ``param_stats``' algorithmic bytes (12 per element: all three tensors present) over the time of its launch pair (HIP
events directly around the C-ABI call, median of 50), as a fraction of the 6.29 TB/s copy rate measured on this device
(SURVEY.md section 6).
(c) The 32x64, B = 32, S = 1 training step of the default model with ``TrainStats`` on and off, eager and as a
HIP-graph replay: device-synchronised wall time per step, the four alternated round by round, median and all rounds (the
spread of the rounds is the yardstick for the on/off difference).

One JSON line, also written to profiles/stats_latency.json.  No thresholds: a measurement.

    python tools/stats_latency.py [--rounds 7] [--steps 5] [--batch 32] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29


def composed_stats(named, grads, moments, device):
    """reference trainer.py:844-917 on device tensors; returns the metrics dict of device scalars (nothing is read)"""
    zero = lambda: torch.zeros((), device=device)      # noqa: E731
    grad_sq, param_sq, momentum_sq, dot = defaultdict(zero), defaultdict(zero), defaultdict(zero), defaultdict(zero)
    for (key, p), g, m in zip(named, grads, moments):
        param_sq[key] = param_sq[key] + (p.detach().float() ** 2).sum()
        if g is not None:
            grad_sq[key] = grad_sq[key] + (g ** 2).sum()
            if m is not None:
                dot[key] = dot[key] + (g * m).sum()
                momentum_sq[key] = momentum_sq[key] + (m ** 2).sum()
    metrics = {"grad/total": torch.stack(list(grad_sq.values()) or [zero()]).sum().sqrt()}
    eps = 1e-12
    total_dot, total_grad_sq, total_momentum_sq = zero(), zero(), zero()
    for k in sorted(grad_sq.keys()):
        gnorm = grad_sq[k].sqrt()
        pnorm = param_sq[k].sqrt().clamp_min(eps)
        metrics[f"grad/{k}"] = gnorm
        metrics[f"gradratio/{k}"] = gnorm / pnorm
        metrics[f"pnorm/{k}"] = pnorm
        # (the reference tests momentum_sq[k] > 0 on the host here: one device read per group, left out in its favour)
        metrics[f"grad_alignment/{k}"] = dot[k] / (grad_sq[k].sqrt() * momentum_sq[k].sqrt() + eps)
        total_dot = total_dot + dot[k]
        total_grad_sq = total_grad_sq + grad_sq[k]
        total_momentum_sq = total_momentum_sq + momentum_sq[k]
    metrics["grad_alignment/total"] = total_dot / (total_grad_sq.sqrt() * total_momentum_sq.sqrt() + eps)
    return metrics


def timed(fn, iters):
    """(host ms per call to enqueue, device ms per call) of ``iters`` back-to-back calls"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * (t1 - t0) / iters, e0.elapsed_time(e1) / iters


def default_model(H=32, W=64):
    from paradis_model_amd.config import default_config, stub_datamodule
    from paradis_model_amd.harness import make_grids
    from paradis_model_amd.model import Paradis
    cfg = default_config()
    lat, lg, og = make_grids(H, W, False)
    torch.manual_seed(42)
    return cfg, lat, Paradis(stub_datamodule(cfg), cfg, lg, og).cuda()


def stats_times(rounds, iters_kernel, iters_composed):
    from paradis_model_amd import _lib
    from paradis_model_amd.diagnostics import StatsPlan, group_key, param_stats
    cfg, _, model = default_model()
    names = [n for n, _ in model.named_parameters()]
    params = [p.detach() for _, p in model.named_parameters()]
    g = torch.Generator(device="cuda").manual_seed(3)
    grads = [torch.randn(p.shape, device="cuda", generator=g) * 1e-3 for p in params]
    moments = [0.5 * gr + 3e-4 * torch.randn(gr.shape, device="cuda", generator=g) for gr in grads]
    keys = [group_key(n) for n in names]
    order = sorted(set(keys))
    groups = [order.index(k) for k in keys]
    plan = StatsPlan([p.numel() for p in params], groups, len(order), "cuda")
    named = list(zip(keys, params))
    fns = {"param_stats": (lambda: param_stats(params, grads, moments, groups, plan=plan), iters_kernel),
           "composed": (lambda: composed_stats(named, grads, moments, "cuda"), iters_composed)}
    with torch.no_grad():
        for fn, _ in fns.values():
            for _ in range(3):
                fn()
        host, dev = {k: [] for k in fns}, {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, iters) in fns.items():
                h, d = timed(fn, iters)
                host[k].append(h)
                dev[k].append(d)
        # a single call on an idle device: the host time to enqueue it when nothing is queued in front (a back-to-back
        # loop of param_stats waits, call by call, for the previous call's address-table copy: its host time per call is
        # the device's) and the device time including that copy
        single, single_host = {k: [] for k in fns}, {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, _) in fns.items():
                h, d = timed(fn, 1)
                single_host[k].append(h)
                single[k].append(d)
        # the launch pair alone: HIP events directly around the C-ABI call (no address-table copy, no host in between)
        prof = _lib.PROFILER = _lib.LaunchProfiler()
        for _ in range(50):
            fns["param_stats"][0]()
        torch.cuda.synchronize()
        _lib.PROFILER = None
        rec = prof.records["param_stats"]
        pair_ms = sorted(a.elapsed_time(b) for a, b in rec[1])
        out = plan.out.cpu().double()
        ref = composed_stats(named, grads, moments, "cuda")
    worst = 0.0
    for gi, k in enumerate(order + ["total"]):
        for col, name in ((4, "grad"), (7, "grad_alignment")):
            want = float(ref[f"{name}/{k}"])
            worst = max(worst, abs(float(out[gi, col]) - want) / abs(want))
    med = statistics.median
    n_el = sum(p.numel() for p in params)
    nbytes = 12.0 * n_el
    t = med(pair_ms)
    rate = nbytes / (t * 1e-3) / 1e12
    r5 = lambda v: [round(x, 5) for x in v]      # noqa: E731
    return {"tensors": len(params), "elements": n_el, "groups": order, "chunks": plan.n_chunks, "rounds": rounds,
            "iters": {"param_stats": iters_kernel, "composed": iters_composed},
            "param_stats_host_ms": round(med(host["param_stats"]), 5), "composed_host_ms": round(med(host["composed"]), 5),
            "param_stats_device_ms": round(med(dev["param_stats"]), 5), "composed_device_ms": round(med(dev["composed"]), 5),
            "param_stats_single_call_host_ms": round(med(single_host["param_stats"]), 5),
            "composed_single_call_host_ms": round(med(single_host["composed"]), 5),
            "param_stats_single_call_device_ms": round(med(single["param_stats"]), 5),
            "composed_single_call_device_ms": round(med(single["composed"]), 5),
            "param_stats_launch_pair_ms": round(t, 5), "param_stats_launch_pair_ms_min_max": [round(pair_ms[0], 5), round(pair_ms[-1], 5)],
            "param_stats_host_ms_all": r5(host["param_stats"]), "composed_host_ms_all": r5(host["composed"]),
            "param_stats_device_ms_all": r5(dev["param_stats"]), "composed_device_ms_all": r5(dev["composed"]),
            "algorithmic_MB": round(nbytes / 1e6, 2), "param_stats_TBps": round(rate, 3),
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3), "param_stats_vs_composed_max_rel": worst}


def step_times(B, S, rounds, steps):
    from paradis_model_amd.config import feature_layout
    from paradis_model_amd.diagnostics import TrainStats
    from paradis_model_amd.harness import GraphedTrainStep, TrainStep, synthetic_batch
    from paradis_model_amd.loss import build_loss
    H, W = 32, 64
    batch = synthetic_batch(H, W, False, B, S, seed=1234, device="cuda")
    runs, last = {}, {}
    for graphed in (False, True):
        for stats in (False, True):
            cfg, lat, model = default_model(H, W)
            lay = feature_layout(cfg)
            loss = build_loss(cfg, lat).cuda()
            ts = TrainStats(model, loss) if stats else None
            step = TrainStep(model, loss, cfg, num_common=lay.num_common_features, n_inputs=cfg.dataset.n_time_inputs,
                             capturable=graphed, stats=ts)
            fn = GraphedTrainStep(step, batch, warmup=2) if graphed else step
            for _ in range(3):
                fn(batch)
            torch.cuda.synchronize()
            runs[("graph" if graphed else "eager") + ("_stats" if stats else "")] = (fn, ts)
    wall = {k: [] for k in runs}
    host = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, ts) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn(batch)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[k].append(1e3 * (t1 - t0) / steps)
            wall[k].append(1e3 * (t2 - t0) / steps)
            if ts is not None:
                last[k] = ts.result()
    med = statistics.median
    res = {"model": "default", "grid": f"{H}x{W}", "B": B, "S": S, "rounds": rounds, "steps_per_round": steps}
    for k in runs:
        res[k + "_ms"] = round(med(wall[k]), 3)
        res[k + "_host_ms"] = round(med(host[k]), 3)
        res[k + "_ms_all"] = [round(v, 3) for v in wall[k]]
    res["eager_stats_minus_off_ms"] = round(res["eager_stats_ms"] - res["eager_ms"], 3)
    res["graph_stats_minus_off_ms"] = round(res["graph_stats_ms"] - res["graph_ms"], 3)
    res["spread_ms"] = {k: round(max(wall[k]) - min(wall[k]), 3) for k in runs}
    res["logged_keys"] = {k: len(v) for k, v in last.items()}
    res["grad_total"] = {k: v["grad/total"] for k, v in last.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rollout", type=int, default=1)
    ap.add_argument("--no-step", action="store_true", help="the statistics times only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stats_latency.py needs the GPU")
    from paradis_model_amd import ops
    res = {"tool": "stats_latency", "device": torch.cuda.get_device_name(0), "gemm": ops.gemm_scheme_name(),
           "copy_rate_TBps": COPY_TBPS}
    res["stats"] = stats_times(a.rounds, 200, 10)
    if not a.no_step:
        res["step"] = step_times(a.batch, a.rollout, a.rounds, a.steps)
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "stats_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
