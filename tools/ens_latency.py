"""Ensemble-verification latency on the MI355X.

``ensemble.EnsembleCard.update`` (one launch pair of ``csrc/ensemble.hip``) on the shipped 96-channel chunk, at one
721x1440 ensemble (G = 1) of M = 4, 16 and ``paradis_ens_max_members()`` members, and at 32x64 with G * M = 32, against

  (a) an ATen ``copy_`` of as many bytes as the launch reads (4 (M + 1) per cell and channel), and
  (b) the same row sums and rank counts composed from ATen ops on the same device: a ``sort`` along the member axis for
      the pair term (sum_i (2 i - M + 1) x_(i)), differences, means and comparisons, and a ``bincount`` for the histogram,

HIP-event time per call, the three alternated in one process.  The update's algorithmic bytes over its time are also
given as a fraction of the 6.29 TB/s copy rate measured on this device.  The composed integers
must equal the kernel's (``ints_equal``; ``ints_differ`` counts the entries that do not); the composed sums agree to
fp32 rounding (``sums_max_rel``: the composition sums in another order and through the sort identity).

Every timed configuration runs in a child process of its own under its own time limit; after a child that failed or ran
out of time nothing more is started.

One JSON line, also written to profiles/ens_latency.json (``--out``).  No thresholds: a measurement.

    python tools/ens_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
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


def composed(f, t, M):
    """(sums double [C, H, 4], counts int64 [C, H, 2 + M]) of the first update of a card with seed 0 at lead 0, from
    ATen ops (what a user composes without the kernel); the few tied cells get the card's hash ranks"""
    import torch
    G, Cc, H, W = t.shape
    x = f.view(G, M, Cc, H, W)
    y = t.unsqueeze(1)
    valid = torch.isfinite(t) & torch.isfinite(x).all(dim=1)
    A = (x - y).abs().sum(dim=1)
    coef = (2.0 * torch.arange(M, device=f.device, dtype=torch.float32) - (M - 1)).view(1, M, 1, 1, 1)
    P = (x.sort(dim=1).values * coef).sum(dim=1)
    m = x.mean(dim=1)
    E2 = (m - t) ** 2
    V = ((x - m.unsqueeze(1)) ** 2).sum(dim=1)
    lo = (x < y).sum(dim=1)
    eq = (x == y).sum(dim=1)
    idx = torch.arange(G * Cc * H * W, device=f.device).view(G, Cc, H, W)          # ((g C + c) H + h) W + w: the hash key
    lo = lo + hash32(idx) % (eq + 1)
    zero = torch.zeros((), device=f.device)
    sums = torch.stack([torch.where(valid, v, zero).double().sum(dim=(0, 3)) for v in (A, P, E2, V)], dim=-1)
    row = (torch.arange(Cc * H, device=f.device).view(1, Cc, H, 1) * (M + 1) + lo)[valid]
    hist = torch.bincount(row, minlength=Cc * H * (M + 1)).view(Cc, H, M + 1)
    return sums, torch.cat([valid.sum(dim=(0, 3)).unsqueeze(-1), hist], dim=-1)


def hash32(x):
    """the tie-breaking hash of ensemble.py on int64 tensors holding uint32 values"""
    mask = 0xFFFFFFFF
    x = x & mask
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & mask
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & mask
    return x ^ (x >> 16)


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(G, M, H, W, rounds, iters, iters_composed):
    import torch
    from paradis_model_amd.ensemble import EnsembleCard
    if not torch.cuda.is_available():
        raise SystemExit("ens_latency.py needs the GPU")
    g = torch.Generator(device="cuda").manual_seed(11)
    true = torch.randn(G * M, C, H, W, device="cuda", generator=g)
    t = true[::M]                                      # a view with batch stride M*C*H*W, as Forecaster.run hands it over
    f = torch.randn(G * M, C, H, W, device="cuda", generator=g)
    f.mul_(0.6).add_(0.1).view(G, M, C, H, W).add_(t.unsqueeze(1))
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    card = EnsembleCard([f"c{i}" for i in range(C)], lat, 1, M)
    nbytes = 4 * (M + 1) * G * C * H * W
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fns = {"update": (lambda: card.update(0, f, t), iters), "copy": (lambda: dst.copy_(src), iters),
           "composed": (lambda: composed(f, t, M), iters_composed)}
    with torch.no_grad():
        for fn, _ in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, (fn, n) in fns.items():
                ms[name].append(event_ms(fn, n))
        card.reset()
        card.update(0, f, t)
        sums, ints = composed(f, t, M)
        ints_equal = bool(torch.equal(card.acc_int[0], ints))
        ints_differ = int((card.acc_int[0] != ints).sum())
        rel = ((card.acc_real[0] - sums).abs() / card.acc_real[0].abs().clamp_min(1e-300)).max()
    tm, tc, ta = (statistics.median(ms[n]) for n in ("update", "copy", "composed"))
    rate = nbytes / (tm * 1e-3) / 1e12
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "G": G, "M": M, "C": C, "iters": iters,
            "iters_composed": iters_composed, "rounds": rounds, "update_ms": round(tm, 5), "copy_ms": round(tc, 5),
            "composed_ms": round(ta, 5), "update_ms_all": [round(v, 5) for v in ms["update"]],
            "copy_ms_all": [round(v, 5) for v in ms["copy"]], "composed_ms_all": [round(v, 5) for v in ms["composed"]],
            "algorithmic_MB": round(nbytes / 1e6, 3), "update_TBps": round(rate, 3),
            "copy_TBps": round(2 * nbytes / (tc * 1e-3) / 1e12, 3),          # a copy reads and writes its bytes
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3), "update_over_copy": round(tm / tc, 3),
            "composed_over_update": round(ta / tm, 1), "ints_equal": ints_equal, "ints_differ": ints_differ, "sums_max_rel": float(rel)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one ensemble of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ens_latency.json"))
    ap.add_argument("--one", default="", help="(internal) G,M,H,W,iters,iters_composed: measure one configuration")
    a = ap.parse_args()
    if a.one:
        G, M, H, W, iters, itc = (int(v) for v in a.one.split(","))
        print("RESULT " + json.dumps(measure(G, M, H, W, a.rounds, iters, itc)), flush=True)
        return
    from paradis_model_amd.ensemble import max_members
    mmax = max_members()
    members = sorted({4, 16, mmax})
    configs = [(32 // M, M, 32, 64, 500, 20) for M in members if 32 % M == 0]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        configs = [(1, M, H, W, 50, 3) for M in members] + configs
    res = {"tool": "ens_latency", "copy_rate_TBps": COPY_TBPS, "update": []}
    for cfg in configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", ",".join(str(v) for v in cfg)]
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"ens_latency: {cfg} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"ens_latency: {cfg} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["update"].append(json.loads(line[len("RESULT "):]))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
