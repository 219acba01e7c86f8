"""Forecast-verification latency on the MI355X.

``verify.Scorecard.update`` (one launch pair of ``csrc/verify.hip``) against the same per-sample numbers composed from
ATen ops on the same device - HIP-event time per call, the two alternated in one process - at 32x64 with B = 32 and at
one 721x1440 state, C = 97, with and without a climatology.  The update's algorithmic bytes (12 B C H W with a
climatology, 8 B C H W without) over its time is given as a fraction of the 6.29 TB/s copy rate measured on this device
(SURVEY.md section 6).

Every timed configuration runs in a child process of its own under its own time limit; after a child that failed or ran
out of time nothing more is started.

One JSON line, also written to profiles/verify_latency.json.  No thresholds: a measurement.

    python tools/verify_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
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
C = 97


def lat_weights(H):
    lat = (-90.0 + 90.0 / H + (180.0 / H) * np.arange(H)) * np.pi / 180.0
    w = np.cos(lat)
    return (w / w.mean()).astype(np.float32)


def composed(f, t, w, Z, clim, k):
    """the per-sample scores [B, C] of one update from ATen ops (what a user composes without the kernel)"""
    import torch
    wv = w.view(1, 1, -1, 1)
    d = f - t
    out = [(wv * d * d).sum((-2, -1)) / Z, (wv * d).sum((-2, -1)) / Z, (wv * d.abs()).sum((-2, -1)) / Z]
    if clim is not None:
        cl = clim[k.long()]
        fa, ta = f - cl, t - cl
        ff, tt, ft = ((wv * x).sum((-2, -1)) for x in (fa * fa, ta * ta, fa * ta))
        out += [ft / torch.sqrt(ff * tt), ff, tt]
    return torch.stack(out)


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(B, H, W, with_clim, rounds, iters):
    import torch
    from paradis_model_amd.verify import Scorecard
    if not torch.cuda.is_available():
        raise SystemExit("verify_latency.py needs the GPU")
    g = torch.Generator(device="cuda").manual_seed(11)
    true = torch.randn(B, 2, C, H, W, device="cuda", generator=g)
    t = true[:, 1]                                     # a view with batch stride 2*C*H*W, as a stored truth
    f = t + 0.3 * torch.randn(B, C, H, W, device="cuda", generator=g) + 0.2
    clim = 0.5 * torch.randn(2, C, H, W, device="cuda", generator=g) if with_clim else None
    k = (torch.arange(B, device="cuda") % 2).to(torch.int32) if with_clim else None
    w = torch.from_numpy(lat_weights(H)).cuda()
    Z = float(W) * float(w.double().sum())
    card = Scorecard([f"c{i}" for i in range(C)], w, 1, climatology=clim)
    fns = {"update": lambda: card.update(0, f, t, k), "composed": lambda: composed(f, t, w, Z, clim, k)}
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                ms[name].append(event_ms(fn, iters))
        card.reset()
        card.update(0, f, t, k)
        got = card.result()
        ref = composed(f, t, w, Z, clim, k).double().cpu().numpy()
    rmse_ref = np.sqrt(ref[0].mean(0))
    nbytes = (12.0 if with_clim else 8.0) * B * C * H * W
    tm = statistics.median(ms["update"])
    rate = nbytes / (tm * 1e-3) / 1e12
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "B": B, "C": C,
            "climatology": bool(with_clim), "iters": iters, "rounds": rounds,
            "update_ms": round(tm, 5), "composed_ms": round(statistics.median(ms["composed"]), 5),
            "update_ms_all": [round(v, 5) for v in ms["update"]],
            "composed_ms_all": [round(v, 5) for v in ms["composed"]],
            "algorithmic_MB": round(nbytes / 1e6, 2), "update_TBps": round(rate, 3),
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3),
            "rmse_vs_composed_max_rel": float(np.abs(got["rmse"][0] - rmse_ref).max() / np.abs(rmse_ref).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one state of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--one", default="", help="(internal) B,H,W,with_clim,iters: measure one configuration, print JSON")
    a = ap.parse_args()
    if a.one:
        B, H, W, with_clim, iters = (int(v) for v in a.one.split(","))
        print("RESULT " + json.dumps(measure(B, H, W, with_clim, a.rounds, iters)), flush=True)
        return
    configs = [(32, 32, 64, 2000)]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        configs.append((1, H, W, 200))
    res = {"tool": "verify_latency", "copy_rate_TBps": COPY_TBPS, "update": []}
    for (B, H, W, iters) in configs:
        for with_clim in (1, 0):
            cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one",
                   f"{B},{H},{W},{with_clim},{iters}"]
            try:
                out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"verify_latency: {B}x{C}x{H}x{W} clim={with_clim} ran out of its {a.limit} s; stopping")
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"verify_latency: {B}x{C}x{H}x{W} clim={with_clim} ended with {out.returncode}; stopping")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res["update"].append(json.loads(line[len("RESULT "):]))
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "verify_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
