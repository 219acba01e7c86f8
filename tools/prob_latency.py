"""Probabilistic-event-verification latency on the MI355X.

``probability.ProbabilityTable.update`` (one launch pair of ``csrc/probability.hip``) on a four-channel state (tp, u, v,
t), at one 721x1440 ensemble (G = 1) of M = 4, 16 and ``paradis_prob_max_members()`` members - with three sources
(plain, speed, anomaly) of 4 thresholds each ("3x4") and with one plain source of 8 ("1x8") - and at 32x64 with
G * M = 32, against

  (a) an ATen ``copy_`` of as many bytes as the launch reads (4 (M + 1) per cell of a plain source, 8 (M + 1) of a
      speed, 4 (M + 1) + 4 of an anomaly), and
  (b) the same integers composed from ATen ops on the same device: the source values, comparisons against each
      threshold, a sum over the member axis and a ``bincount`` of ``row, o, k``,

HIP-event time per call, the three alternated in one process.  The update's algorithmic bytes over its time are also
given as a fraction of the 6.29 TB/s copy rate measured on this device.  The composed integers
must equal the kernel's (``ints_equal``; ``ints_differ`` counts the entries that do not).

Fields: ``random`` - truth ~ N(0, 1), members = truth + 0.1 + 0.6 N(0, 1), the cells of a wave spread over many bins -
and ``dry`` - all zeros: every cell of a threshold in ONE bin, the case in which 64 lanes of a wave meet in one counter.

Every timed configuration runs in a child process of its own under its own time limit; after a child that failed or ran
out of time nothing more is started.

One JSON line, also written to profiles/prob_latency.json (``--out``).  No thresholds: a measurement.

    python tools/prob_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29
NAMES = ["tp", "u", "v", "t"]
EVENT_SETS = {
    "3x4": {"wet": {"source": "tp", "thresholds": [-1.0, 0.0, 0.5, 1.5]},
            "wind": {"source": ("speed", "u", "v"), "thresholds": [0.5, 1.0, 1.5, 2.5]},
            "warm": {"source": ("anomaly", "t"), "thresholds": [-1.0, 0.0, 0.5, 1.5]}},
    "1x8": {"wet": {"source": "tp", "thresholds": [-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]}},
}
# the estimate made from the code before the first run: bytes at ensemble.hip's measured
# 4.9 TB/s for M = 16 at 721x1440
ESTIMATE = {"plain_source_M16_us": 14.4, "3x4_M16_us": 58.5, "assumed_TBps": 4.9}


def composed(table, f, t, clim):
    """the accumulator rows int64 [S, H, 1 + 2 T (M + 1)] of one update (every ensemble in slot 0) from ATen ops: what
    a user composes without the kernel"""
    import torch
    M, T = table.members, table.T
    G, _, H, W = t.shape
    x = f.view(G, M, len(NAMES), H, W)
    out = torch.zeros(len(table.labels), H, 1 + 2 * T * (M + 1), dtype=torch.int64, device=f.device)
    rows = torch.arange(H, device=f.device).view(1, H, 1)
    for s, (kind, (_, c0, c1, nthr)) in enumerate(zip(table.kinds, table._src.tolist())):
        sign = float(table._thr[s, 0])
        if kind == 0:
            vt, vm = t[:, c0], x[:, :, c0]
            valid = torch.isfinite(vt) & torch.isfinite(vm).all(dim=1)
        elif kind == 1:
            vt = (t[:, c0] * t[:, c0] + t[:, c1] * t[:, c1]).sqrt()
            vm = (x[:, :, c0] * x[:, :, c0] + x[:, :, c1] * x[:, :, c1]).sqrt()
            valid = torch.isfinite(t[:, c0]) & torch.isfinite(t[:, c1]) & torch.isfinite(x[:, :, c0]).all(dim=1) & \
                torch.isfinite(x[:, :, c1]).all(dim=1)
        else:
            cl = clim[0, c0].unsqueeze(0)
            vt, vm = t[:, c0] - cl, x[:, :, c0] - cl.unsqueeze(1)
            valid = torch.isfinite(t[:, c0]) & torch.isfinite(cl) & torch.isfinite(x[:, :, c0]).all(dim=1)
        out[s, :, 0] = valid.sum(dim=(0, 2))
        for j in range(nthr):
            thr = float(table._thr[s, 1 + j])
            o = (sign * vt >= thr).long()
            k = (sign * vm >= thr).sum(dim=1)
            bins = ((rows * 2 + o) * (M + 1) + k)[valid]
            hist = torch.bincount(bins, minlength=H * 2 * (M + 1)).view(H, 2 * (M + 1))
            out[s, :, 1 + j * 2 * (M + 1):1 + (j + 1) * 2 * (M + 1)] = hist
    return out


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(G, M, H, W, events, field, rounds, iters, iters_composed):
    import torch
    from paradis_model_amd.probability import ProbabilityTable, bytes_per_cell
    if not torch.cuda.is_available():
        raise SystemExit("prob_latency.py needs the GPU")
    C = len(NAMES)
    g = torch.Generator(device="cuda").manual_seed(11)
    if field == "dry":
        true = torch.zeros(G * M, C, H, W, device="cuda")
        f = torch.zeros(G * M, C, H, W, device="cuda")
        clim = torch.zeros(1, C, H, W, device="cuda")
    else:
        true = torch.randn(G * M, C, H, W, device="cuda", generator=g)
        f = torch.randn(G * M, C, H, W, device="cuda", generator=g)
        f.mul_(0.6).add_(0.1).view(G, M, C, H, W).add_(true[::M].unsqueeze(1))
        clim = 0.3 * torch.randn(1, C, H, W, device="cuda", generator=g)
    t = true[::M]                                      # a view with batch stride M*C*H*W, as Forecaster.run hands it over
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    table = ProbabilityTable(NAMES, lat, 1, EVENT_SETS[events], M, climatology=clim)
    nbytes = sum(bytes_per_cell(k, M) for k in table.kinds) * G * H * W
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fns = {"update": (lambda: table.update(0, f, t), iters), "copy": (lambda: dst.copy_(src), iters),
           "composed": (lambda: composed(table, f, t, clim), iters_composed)}
    with torch.no_grad():
        for fn, _ in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, (fn, n) in fns.items():
                ms[name].append(event_ms(fn, n))
        table.reset()
        table.update(0, f, t)
        ints = composed(table, f, t, clim)
        ints_equal = bool(torch.equal(table.acc[0], ints))
        ints_differ = int((table.acc[0] != ints).sum())
        joint = table.acc[0, :, :, 1:].reshape(len(table.labels), H, table.T, -1).sum(dim=1)
        bins_used = int((joint > 0).sum(dim=-1).max())
    tm, tc, ta = (statistics.median(ms[n]) for n in ("update", "copy", "composed"))
    rate = nbytes / (tm * 1e-3) / 1e12
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "G": G, "M": M, "events": events,
            "field": field, "bins_used_max": bins_used, "iters": iters, "iters_composed": iters_composed,
            "rounds": rounds, "update_ms": round(tm, 5), "copy_ms": round(tc, 5), "composed_ms": round(ta, 5),
            "update_ms_all": [round(v, 5) for v in ms["update"]], "copy_ms_all": [round(v, 5) for v in ms["copy"]],
            "composed_ms_all": [round(v, 5) for v in ms["composed"]], "algorithmic_MB": round(nbytes / 1e6, 3),
            "update_TBps": round(rate, 3),
            "copy_TBps": round(2 * nbytes / (tc * 1e-3) / 1e12, 3),          # a copy reads and writes its bytes
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3), "update_over_copy": round(tm / tc, 3),
            "composed_over_update": round(ta / tm, 1), "ints_equal": ints_equal, "ints_differ": ints_differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one ensemble of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prob_latency.json"))
    ap.add_argument("--one", default="", help="(internal) G,M,H,W,events,field,iters,iters_composed: one configuration")
    a = ap.parse_args()
    if a.one:
        v = a.one.split(",")
        G, M, H, W = (int(x) for x in v[:4])
        print("RESULT " + json.dumps(measure(G, M, H, W, v[4], v[5], a.rounds, int(v[6]), int(v[7]))), flush=True)
        return
    from paradis_model_amd.probability import max_members
    mmax = max_members()
    members = sorted({4, 16, mmax})
    configs = [(32 // M, M, 32, 64, "3x4", "random", 500, 20) for M in members if 32 % M == 0]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        big = [(1, M, H, W, ev, "random", 100, 3) for ev in ("3x4", "1x8") for M in members]
        big += [(1, 16, H, W, ev, "dry", 100, 3) for ev in ("3x4", "1x8")]
        configs = big + configs
    res = {"tool": "prob_latency", "copy_rate_TBps": COPY_TBPS, "estimate_before_the_first_run": ESTIMATE, "update": []}
    for cfg in configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", ",".join(str(v) for v in cfg)]
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"prob_latency: {cfg} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"prob_latency: {cfg} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["update"].append(json.loads(line[len("RESULT "):]))
        sys.stderr.write(f"prob_latency: {cfg}: {res['update'][-1]['update_ms']} ms\n")
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
