"""Latency of global-norm gradient clipping on the MI355X: ``clip.clip_grad_norm_`` (csrc/clip.hip, three launches behind one
address-row copy) against the ATen path it replaces, ``torch.nn.utils.clip_grad_norm_(..., foreach=True)``, on the default
model's 335 gradient shapes (tests/golden/default_manifest.json; seeded gradients, no model is built).

For each path, once with a ``max_norm`` that clips and once with one that does not: the host time to enqueue one call and
the device time per call (HIP events around ``iters`` back-to-back calls), the paths alternated round by round in one
process; the number of device kernels one call launches (torch.profiler); and for the HIP path the time of the three
launches alone (HIP events directly around the C-ABI call, median of 50) as GB/s against 12 bytes per element (4 read by the
norm pass, 8 moved by the scale pass; when nothing is clipped the scale pass returns at once, so the bytes really moved are
4 per element: both rates are given) and as a fraction of the 6.29 TB/s copy rate measured on this device (SURVEY.md
section 6).  The 240 MB of gradients fit in the 256 MB Infinity Cache, so back-to-back calls read them from there; the
"cold" figures are taken with a 1 GiB buffer rewritten in front of every call (events around the call only).

A clipped gradient has the norm ``max_norm``, so the same ``max_norm`` clips once only: the "clips" case lowers it by
0.1 % per call.

One JSON line, also written to profiles/clip_latency.json.  No thresholds: a measurement.

    python tools/clip_latency.py [--rounds 7] [--iters 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29


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


def kernels_per_call(fn):
    """device kernels (and memcpy / memset activities) of one call, by torch.profiler; ``None`` if it cannot tell"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:          # a measurement that is not available is reported as such, not guessed
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_latency.py needs the GPU")
    from paradis_model_amd import _lib, clip
    with open(os.path.join(ROOT, "tests", "golden", "default_manifest.json")) as f:
        shapes = [tuple(shape) for _, shape in json.load(f)["entries"]]
    g = torch.Generator(device="cuda").manual_seed(3)
    params = []
    for shape in shapes:
        p = torch.nn.Parameter(torch.empty(shape, device="cuda"))
        p.grad = torch.randn(shape, device="cuda", generator=g) * 1e-3
        params.append(p)
    n_el = sum(p.numel() for p in params)
    plan = clip.ClipPlan([p.numel() for p in params], "cuda")
    norm0 = float(torch.nn.utils.clip_grad_norm_(params, 1e30))
    state = {"max_norm": 0.5 * norm0}

    def next_max_norm(case):
        if case == "does_not_clip":
            return 1e30
        state["max_norm"] *= 0.999           # below the norm the previous call left: this call clips too
        return state["max_norm"]

    cases = ("clips", "does_not_clip")
    fns = {}
    for case in cases:
        fns[("hip", case)] = lambda case=case: clip.clip_grad_norm_(params, next_max_norm(case), plan=plan)
        fns[("aten", case)] = lambda case=case: torch.nn.utils.clip_grad_norm_(params, next_max_norm(case), foreach=True)
    for fn in fns.values():
        for _ in range(3):
            fn()
    # agreement of the two paths on the same gradients (the norm; both leave the scaled gradients behind)
    want = float(torch.nn.utils.clip_grad_norm_(params, 1e30, foreach=True))
    got = float(clip.clip_grad_norm_(params, 1e30, plan=plan)[0])
    host, dev = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            h, d = timed(fn, a.iters)
            host[k].append(h)
            dev[k].append(d)
    launches = {k: kernels_per_call(fn) for k, fn in fns.items()}
    # the three launches alone: HIP events directly around the C-ABI call (no address-row copy, no host in between)
    alone, cold, coefs = {}, {}, {}
    flush = torch.zeros(1 << 28, device="cuda")           # 1 GiB: four times the Infinity Cache
    for case in cases:
        for store, flushed in ((alone, False), (cold, True)):
            prof = _lib.PROFILER = _lib.LaunchProfiler()
            for _ in range(50):
                if flushed:
                    flush.add_(1.0)
                fns[("hip", case)]()
            torch.cuda.synchronize()
            _lib.PROFILER = None
            store[case] = sorted(x.elapsed_time(y) for x, y in prof.records["clip_grad_norm"][1])
        coefs[case] = float(plan.out[1])
    med = statistics.median
    res = {"tool": "clip_latency", "device": torch.cuda.get_device_name(0), "tensors": len(params), "elements": n_el,
           "chunks": plan.n_chunks, "rounds": a.rounds, "iters": a.iters, "copy_rate_TBps": COPY_TBPS,
           "algorithmic_MB_at_12B": round(12.0 * n_el / 1e6, 2), "norm_hip_vs_aten_rel": abs(got - want) / want}
    for (path, case), fn in fns.items():
        key = f"{path}_{case}"
        res[key] = {"device_us": round(1e3 * med(dev[(path, case)]), 2), "host_us": round(1e3 * med(host[(path, case)]), 2),
                    "device_us_all": [round(1e3 * v, 2) for v in dev[(path, case)]],
                    "device_activities_per_call": launches[(path, case)]}
    for case, ms in alone.items():
        t = med(ms) * 1e-3
        entry = res[f"hip_{case}"]
        entry["three_launches_us"] = round(1e6 * t, 2)
        entry["three_launches_us_min_max"] = [round(1e3 * ms[0], 2), round(1e3 * ms[-1], 2)]
        entry["GBps_at_12B"] = round(12.0 * n_el / t / 1e9, 1)
        entry["fraction_of_copy_rate_at_12B"] = round(12.0 * n_el / t / 1e12 / COPY_TBPS, 3)
        tc = med(cold[case]) * 1e-3
        entry["three_launches_cold_us"] = round(1e6 * tc, 2)
        entry["three_launches_cold_us_min_max"] = [round(1e3 * cold[case][0], 2), round(1e3 * cold[case][-1], 2)]
        entry["cold_GBps_at_12B"] = round(12.0 * n_el / tc / 1e9, 1)
        entry["cold_fraction_of_copy_rate_at_12B"] = round(12.0 * n_el / tc / 1e12 / COPY_TBPS, 3)
        entry["last_coefficient"] = coefs[case]
        if case == "does_not_clip":
            entry["GBps_at_4B_moved"] = round(4.0 * n_el / t / 1e9, 1)
            entry["cold_GBps_at_4B_moved"] = round(4.0 * n_el / tc / 1e9, 1)
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "clip_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
