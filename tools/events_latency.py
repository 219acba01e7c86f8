"""Event-verification latency on the MI355X.

``events.EventTable.update`` (one launch pair of ``csrc/events.hip``) on the shipped 96-channel chunk, at one 721x1440
state and at 32x64 with B = 32, for two sets of sources - three sources (plain precipitation, 10 m wind speed and a 2 m
temperature anomaly, 4 thresholds each) and one plain source with 8 thresholds - against

  (a) an ATen ``copy_`` of as many bytes as the launch reads (8 per cell of a plain source, 16 of a speed, 12 of an
      anomaly), and
  (b) the same integer rows composed from ATen comparisons, ``logical_and`` and row sums on the same device,

HIP-event time per call, the three alternated in one process.  The update's algorithmic bytes over its time are also
given as a fraction of the 6.29 TB/s copy rate measured on this device, the figure
``tools/verify_latency.py`` reports for ``verify.hip``.  The composed rows must equal the kernel's (``rows_equal``).

Every timed configuration runs in a child process of its own under its own time limit; after a child that failed or ran
out of time nothing more is started.

One JSON line, also written to profiles/events_latency.json (``--out``).  No thresholds: a measurement.

    python tools/events_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
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
C = 96
TP, U10, V10, T2M = "c95", "c90", "c91", "c92"
SOURCE_SETS = {
    "three_x4": {"rain": {"source": TP, "thresholds": [0.25, 0.75, 1.25, 2.0]},
                 "wind": {"source": ("speed", U10, V10), "thresholds": [0.875, 1.375, 2.125, 3.0]},
                 "warm": {"source": ("anomaly", T2M), "thresholds": [-1.5, -0.5, 0.5, 1.5]}},
    "one_x8": {"rain": {"source": TP, "thresholds": [-1.5, -1.0, -0.5, 0.0, 0.25, 0.75, 1.25, 2.0]}},
}


def composed(table, f, t, clim, k):
    """the integer rows of one update from ATen ops: per source [H, 1 + 3 nthr] int64 (what a user composes without the
    kernel: a comparison, a logical_and and a row sum per threshold and class)"""
    import torch
    out = []
    for s, kind in enumerate(table.kinds):
        _, c0, c1, n = (int(v) for v in table._src[s])
        if kind == 0:
            xf, xt = f[:, c0], t[:, c0]
            valid = torch.isfinite(xf) & torch.isfinite(xt)
        elif kind == 1:
            xf = torch.sqrt(f[:, c0] * f[:, c0] + f[:, c1] * f[:, c1])
            xt = torch.sqrt(t[:, c0] * t[:, c0] + t[:, c1] * t[:, c1])
            valid = torch.isfinite(f[:, c0]) & torch.isfinite(f[:, c1]) & torch.isfinite(t[:, c0]) & torch.isfinite(t[:, c1])
        else:
            cl = clim[k.long(), c0]
            xf, xt = f[:, c0] - cl, t[:, c0] - cl
            valid = torch.isfinite(f[:, c0]) & torch.isfinite(t[:, c0]) & torch.isfinite(cl)
        sign = float(table._thr[s, 0])
        cols = [valid.sum((0, 2))]
        Fs, Os = [], []
        for j in range(n):
            thr = float(table._thr[s, 1 + j])
            Fs.append(valid & (sign * xf >= thr))
            Os.append(valid & (sign * xt >= thr))
        cols += [F.sum((0, 2)) for F in Fs] + [O.sum((0, 2)) for O in Os]
        cols += [torch.logical_and(F, O).sum((0, 2)) for F, O in zip(Fs, Os)]
        out.append(torch.stack(cols, dim=1))
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


def measure(B, H, W, which, rounds, iters):
    import torch
    from paradis_model_amd.events import EventTable
    if not torch.cuda.is_available():
        raise SystemExit("events_latency.py needs the GPU")
    g = torch.Generator(device="cuda").manual_seed(11)
    true = torch.randn(B, 2, C, H, W, device="cuda", generator=g)
    t = true[:, 1]                                     # a view with batch stride 2*C*H*W, as a stored truth
    f = t + 0.6 * torch.randn(B, C, H, W, device="cuda", generator=g) + 0.1
    clim = 0.5 * torch.randn(2, C, H, W, device="cuda", generator=g)
    k = (torch.arange(B, device="cuda") % 2).to(torch.int32)
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    table = EventTable([f"c{i}" for i in range(C)], lat, 1, SOURCE_SETS[which], climatology=clim)
    nbytes = int(table._bytes_per_cell) * B * H * W
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fns = {"update": lambda: table.update(0, f, t, k), "copy": lambda: dst.copy_(src),
           "composed": lambda: composed(table, f, t, clim, k)}
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                ms[name].append(event_ms(fn, iters))
        table.reset()
        table.update(0, f, t, k)
        ref = composed(table, f, t, clim, k)
        acc = table.acc[0]
        TM = table.tmax
        equal = True
        for s, n in enumerate(table.n_thresholds):
            cols = [0] + [1 + j for j in range(n)] + [1 + TM + j for j in range(n)] + [1 + 2 * TM + j for j in range(n)]
            equal = equal and bool(torch.equal(acc[s][:, cols], ref[s]))
    tm, tc, ta = (statistics.median(ms[n]) for n in ("update", "copy", "composed"))
    rate = nbytes / (tm * 1e-3) / 1e12
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "B": B, "C": C, "sources": which,
            "iters": iters, "rounds": rounds, "update_ms": round(tm, 5), "copy_ms": round(tc, 5),
            "composed_ms": round(ta, 5), "update_ms_all": [round(v, 5) for v in ms["update"]],
            "copy_ms_all": [round(v, 5) for v in ms["copy"]], "composed_ms_all": [round(v, 5) for v in ms["composed"]],
            "algorithmic_MB": round(nbytes / 1e6, 3), "update_TBps": round(rate, 3),
            "copy_TBps": round(2 * nbytes / (tc * 1e-3) / 1e12, 3),          # a copy reads and writes its bytes
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3), "copy_over_update": round(tc / tm, 3),
            "composed_over_update": round(ta / tm, 1), "rows_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one state of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_latency.json"))
    ap.add_argument("--one", default="", help="(internal) B,H,W,sources,iters: measure one configuration, print JSON")
    a = ap.parse_args()
    if a.one:
        B, H, W, which, iters = a.one.split(",")
        print("RESULT " + json.dumps(measure(int(B), int(H), int(W), which, a.rounds, int(iters))), flush=True)
        return
    configs = [(32, 32, 64, 1000)]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        configs.insert(0, (1, H, W, 200))
    res = {"tool": "events_latency", "copy_rate_TBps": COPY_TBPS, "update": []}
    for (B, H, W, iters) in configs:
        for which in SOURCE_SETS:
            cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one",
                   f"{B},{H},{W},{which},{iters}"]
            try:
                out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"events_latency: {B}x{C}x{H}x{W} {which} ran out of its {a.limit} s; stopping")
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"events_latency: {B}x{C}x{H}x{W} {which} ended with {out.returncode}; stopping")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res["update"].append(json.loads(line[len("RESULT "):]))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
