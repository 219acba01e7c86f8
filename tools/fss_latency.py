"""Neighbourhood-verification latency on the MI355X.

``neighbourhood.FractionsTable.update`` (three launches of ``csrc/fss.hip``) on the shipped 96-channel chunk with the
scales ``[0, 2, 4, 8, 16]``: one 721x1440 state with three sources of 4 thresholds (plain precipitation, 10 m wind speed,
a 2 m temperature anomaly: the sets of ``tools/events_latency.py``) under ``lon_scaling="cells"`` and ``"metric"``, the
same state with one plain source of 8 thresholds, and 32x64 with B = 32 - each against

  (a) an ATen ``copy_`` of as many bytes as the launch reads from the states (8 per cell of a plain source, 16 of a
      speed, 12 of an anomaly), and
  (b) the same integers composed from ATen on the same device: comparisons, a zero-padded column-of-ones ``conv2d`` for
      the clipped latitude window, a circular pad, ``cumsum`` and two gathers for the longitude window of each row's own
      width, squares and products, row sums,

HIP-event time per call, the three alternated in one process.  The composed sums must equal the kernel's
(``rows_equal``).  Also given: the centre rows R a workgroup of the window kernel owns and, per scale, the read
amplification of its halo, (R + 2 ny) / R - of the two-byte decided bits, not of the states, which are read once.

Every timed leg runs in a child process of its own under its own time limit; after a child that failed or ran out of
time nothing more is started.

One JSON line, also written to profiles/fss_latency.json (``--out``).  No thresholds: a measurement.

    python tools/fss_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
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

from tools.events_latency import C, COPY_TBPS, SOURCE_SETS, event_ms  # noqa: E402

SCALES = [0, 2, 4, 8, 16]


def composed(table, f, t, clim, k):
    """the integer sums of one update from ATen ops: per source int64 [H, K, nthr, 3] = (FF, OO, FO)"""
    import torch
    import torch.nn.functional as TF
    B, _, H, W = f.shape
    cap = (W - 1) // 2
    col = torch.arange(W, device=f.device)[None, :]
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
        thr = [float(table._thr[s, 1 + j]) for j in range(n)]
        bits = torch.stack([valid & (sign * xf >= v) for v in thr] + [valid & (sign * xt >= v) for v in thr], dim=1)
        planes = bits.float().reshape(B * 2 * n, 1, H, W)
        per_scale = []
        for ki, ny in enumerate(table.scales):
            ones = torch.ones(1, 1, 2 * ny + 1, 1, device=f.device)
            vert = TF.conv2d(planes, ones, padding=(ny, 0))                       # zero padding: the clipped window
            cs = torch.cumsum(TF.pad(vert, (cap + 1, cap, 0, 0), mode="circular"), dim=-1)
            nx = table._half_x_dev[str(f.device)][ki].long()[:, None]              # [H, 1]
            hi = (col + cap + 1 + nx).expand(B * 2 * n, 1, H, W)
            lo = (col + cap - nx).expand(B * 2 * n, 1, H, W)
            cnt = (torch.gather(cs, -1, hi) - torch.gather(cs, -1, lo)).reshape(B, 2, n, H, W).double()
            cF, cO = cnt[:, 0], cnt[:, 1]
            per_scale.append(torch.stack([(cF * cF).sum((0, 3)), (cO * cO).sum((0, 3)), (cF * cO).sum((0, 3))], dim=-1))
        out.append(torch.stack(per_scale, dim=0).permute(2, 0, 1, 3).long())      # [K, n, H, 3] -> [H, K, n, 3]
    return out


def measure(B, H, W, which, lon_scaling, rounds, iters):
    import torch
    from paradis_model_amd import _lib
    from paradis_model_amd.neighbourhood import FractionsTable
    if not torch.cuda.is_available():
        raise SystemExit("fss_latency.py needs the GPU")
    g = torch.Generator(device="cuda").manual_seed(11)
    true = torch.randn(B, 2, C, H, W, device="cuda", generator=g)
    t = true[:, 1]                                     # a view with batch stride 2*C*H*W, as a stored truth
    f = t + 0.6 * torch.randn(B, C, H, W, device="cuda", generator=g) + 0.1
    clim = 0.5 * torch.randn(2, C, H, W, device="cuda", generator=g)
    k = (torch.arange(B, device="cuda") % 2).to(torch.int32)
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    table = FractionsTable([f"c{i}" for i in range(C)], lat, W, 1, SOURCE_SETS[which], SCALES, lon_scaling=lon_scaling,
                           climatology=clim)
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
                ms[name].append(event_ms(fn, max(1, iters // 20) if name == "composed" else iters))
        table.reset()
        table.update(0, f, t, k)
        ref = composed(table, f, t, clim, k)
        acc = table.acc[0]
        TM, head, K = table.tmax, table.head, len(SCALES)
        equal = True
        for s, n in enumerate(table.n_thresholds):
            win = acc[s][:, head:head + 3 * K * TM].reshape(H, K, TM, 3)[:, :, :n]
            equal = equal and bool(torch.equal(win, ref[s]))
    tm, tc, ta = (statistics.median(ms[n]) for n in ("update", "copy", "composed"))
    rate = nbytes / (tm * 1e-3) / 1e12
    R = int(_lib.lib.paradis_fss_rows(W, max(SCALES)))
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "B": B, "C": C, "sources": which,
            "lon_scaling": lon_scaling, "scales": SCALES, "half_x_max": int(table.half_x.max()),
            "half_x_mean": round(float(table.half_x.mean()), 2), "iters": iters, "rounds": rounds,
            "update_ms": round(tm, 5), "copy_ms": round(tc, 5), "composed_ms": round(ta, 5),
            "update_ms_all": [round(v, 5) for v in ms["update"]], "copy_ms_all": [round(v, 5) for v in ms["copy"]],
            "composed_ms_all": [round(v, 5) for v in ms["composed"]], "algorithmic_MB": round(nbytes / 1e6, 3),
            "update_TBps": round(rate, 3), "copy_TBps": round(2 * nbytes / (tc * 1e-3) / 1e12, 3),
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3), "copy_over_update": round(tc / tm, 3),
            "composed_over_update": round(ta / tm, 1), "rows_per_workgroup": R,
            "halo_read_amplification": [round((R + 2 * ny) / R, 3) for ny in SCALES], "rows_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one state of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each leg's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fss_latency.json"))
    ap.add_argument("--one", default="", help="(internal) B,H,W,sources,lon_scaling,iters: measure one leg, print JSON")
    a = ap.parse_args()
    if a.one:
        B, H, W, which, lon_scaling, iters = a.one.split(",")
        print("RESULT " + json.dumps(measure(int(B), int(H), int(W), which, lon_scaling, a.rounds, int(iters))), flush=True)
        return
    legs = [(32, 32, 64, "three_x4", "cells", 1000)]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        legs = [(1, H, W, "three_x4", "cells", 100), (1, H, W, "three_x4", "metric", 100),
                (1, H, W, "one_x8", "cells", 100)] + legs
    res = {"tool": "fss_latency", "copy_rate_TBps": COPY_TBPS, "update": []}
    for (B, H, W, which, lon_scaling, iters) in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one",
               f"{B},{H},{W},{which},{lon_scaling},{iters}"]
        what = f"{B}x{C}x{H}x{W} {which} {lon_scaling}"
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"fss_latency: {what} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"fss_latency: {what} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["update"].append(json.loads(line[len("RESULT "):]))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
