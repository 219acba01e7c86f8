"""Zonal-spectrum latency on the MI355X.

``spectrum.Spectra.update`` (one launch pair of ``csrc/spectrum.hip``) against (a) an ATen ``copy_`` of as many bytes as
the update reads (8 B C H W) and (b) the same per-sample band spectra composed from ``torch.fft.rfft`` and ATen ops on
the same device - HIP-event time per call, the three alternated in one process - at 32x64 with B = 32 and at one
721x1440 state, C = 96, with 1 and 3 latitude bands.  The update's algorithmic bytes over its time is given as a
fraction of the 6.29 TB/s copy rate measured on this device.

Every timed configuration runs in a child process of its own under its own time limit; after a child that failed or ran
out of time nothing more is started.

One JSON line, also written to profiles/spectrum_latency.json.  No thresholds: a measurement.

    python tools/spectrum_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
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
BANDS = {1: None, 3: {"south": (-90.0, -20.0), "tropics": (-20.0, 20.0), "north": (20.0, 90.0)}}


def grid_lat(H):
    return -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)


def composed(f, t, wb, wsum, mult):
    """the per-sample band spectra [B, C, R, K + 1, 3] of one update from torch.fft.rfft and ATen ops (what a user
    composes without the kernel; zero weights are multiplied in)"""
    import torch
    W = f.shape[-1]
    F, T = torch.fft.rfft(f, dim=-1) / W, torch.fft.rfft(t, dim=-1) / W
    p = torch.stack([mult * (F.real ** 2 + F.imag ** 2), mult * (T.real ** 2 + T.imag ** 2),
                     mult * (F.real * T.real + F.imag * T.imag)], dim=-1)
    return torch.einsum("rh,bchkf->bcrkf", wb, p) / wsum.view(1, 1, -1, 1, 1)


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(B, H, W, R, rounds, iters):
    import torch
    from paradis_model_amd import spectrum
    from paradis_model_amd.spectrum import Spectra
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_latency.py needs the GPU")
    g = torch.Generator(device="cuda").manual_seed(11)
    true = torch.randn(B, 2, C, H, W, device="cuda", generator=g)
    t = true[:, 1]                                     # a view with batch stride 2*C*H*W, as a stored truth
    f = 0.8 * t + 0.3 * torch.randn(B, C, H, W, device="cuda", generator=g) + 0.2
    sp = Spectra([f"c{i}" for i in range(C)], grid_lat(H), 1, bands=BANDS[R])
    wb = torch.from_numpy(sp.band_w).float().cuda()
    wsum = wb.sum(1)
    mult = torch.full((W // 2 + 1,), 2.0, device="cuda")
    mult[0] = mult[-1] = 1.0
    src = torch.randn(2, B, C, H, W, device="cuda", generator=g)           # 8 B C H W bytes: what the update reads
    dst = torch.empty_like(src)
    fns = {"update": lambda: sp.update(0, f, t), "copy": lambda: dst.copy_(src),
           "composed": lambda: composed(f, t, wb, wsum, mult)}
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                ms[name].append(event_ms(fn, iters))
        sp.reset()
        sp.update(0, f, t)
        got = sp.acc[0].cpu().numpy()
        ref = composed(f.double(), t.double(), wb.double(), wsum.double(), mult.double()).sum(0).cpu().numpy()
    tot = ref[:, :, 1:, :2].sum(2).max(-1)[:, :, None, None]
    scale = np.sqrt(np.maximum(ref[:, :, 1:, :1], ref[:, :, 1:, 1:2]) * tot)
    nbytes = 8.0 * B * C * H * W
    tm = statistics.median(ms["update"])
    rate = nbytes / (tm * 1e-3) / 1e12
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "B": B, "C": C, "bands": R,
            "schedule": spectrum.schedule(W), "iters": iters, "rounds": rounds,
            "update_ms": round(tm, 5), "copy_ms": round(statistics.median(ms["copy"]), 5),
            "composed_ms": round(statistics.median(ms["composed"]), 5),
            "update_ms_all": [round(v, 5) for v in ms["update"]],
            "copy_ms_all": [round(v, 5) for v in ms["copy"]],
            "composed_ms_all": [round(v, 5) for v in ms["composed"]],
            "algorithmic_MB": round(nbytes / 1e6, 2), "update_TBps": round(rate, 3),
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3),
            "workspace_MB": round(sum(w.numel() * 8 for w in sp._ws.values()) / 1e6, 2),
            "error_vs_composed_fp64": float((np.abs(got[:, :, 1:] - ref[:, :, 1:]) / scale).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one state of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--one", default="", help="(internal) B,H,W,R,iters: measure one configuration, print JSON")
    a = ap.parse_args()
    if a.one:
        B, H, W, R, iters = (int(v) for v in a.one.split(","))
        print("RESULT " + json.dumps(measure(B, H, W, R, a.rounds, iters)), flush=True)
        return
    configs = [(32, 32, 64, 500)]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        configs.append((1, H, W, 20))
    res = {"tool": "spectrum_latency", "copy_rate_TBps": COPY_TBPS, "update": []}
    for (B, H, W, iters) in configs:
        for R in (1, 3):
            cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one",
                   f"{B},{H},{W},{R},{iters}"]
            try:
                out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"spectrum_latency: {B}x{C}x{H}x{W} R={R} ran out of its {a.limit} s; stopping")
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"spectrum_latency: {B}x{C}x{H}x{W} R={R} ended with {out.returncode}; stopping")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res["update"].append(json.loads(line[len("RESULT "):]))
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "spectrum_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
