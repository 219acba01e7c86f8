"""Quantile-climatology latency on the MI355X (paradis_model_amd/climatology.py ``clim_quantile``, csrc/quantile.hip
``paradis_clim_quantile`` / ``paradis_clim_quantile_packed``).

The three configurations of tools/clim_latency.py, each with a float32 and a ``packing="u16"`` store of F = 9 features,
all of them built, three levels (0.05, 0.5, 0.95) per case:
  32x64, 4 years 6-hourly (T = 5844), all 366 x 4 = 1464 slots, window 1   (about 4 entries per slot)
  the same store, window 61                                               (about 240 entries per slot)
  721x1440, T = 32 rows 6-hourly, the 2 x 4 slots of two days, window 3
HIP-event time of the one launch, against three references on the same device, alternated in one process:
  copy      an ATen ``copy_`` that moves the same algorithmic bytes (half of them read, half written), 2 GiB at the
            most: the rates are compared
  mean      ``clim_mean`` on the same lists (unit weights): what the streaming sum of the same rows costs
  composed  the same quantiles from ATen ops, slot by slot: ``index_select`` of the slot's rows (of a decoded float32
            copy for a packed store; the decode itself is not charged), non-finite values to NaN, ``sort`` along the
            entries (NaN last), the count of kept values, two ``gather``s and the lerp in double.  At 32x64 it runs
            over the first 48 slots and is reported per slot.
GB/s are algorithmic bytes over time: N*C*H*W*(4 | 2) read + Q*K*C*H*W*4 written.

Every case runs in a child process of its own under its own time limit; after a child that failed or ran out of time
nothing more is started.  One JSON line, also written to profiles/quantile_latency.json.  No thresholds.

    python tools/quantile_latency.py [--rounds 5] [--limit 240]
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

F = 9
LEVELS = [0.05, 0.5, 0.95]
COPY_CAP = 1 << 31        # bytes moved by the reference copy_ at the most; its rate is what is compared
# name -> (H, W, first time, rows, plan arguments, iterations per round of the kernel, slots of the composed reference)
CONFIGS = {
    "32x64_w1": (32, 64, "2016-01-01T00", 5844, dict(window_days=1), 20, 48),
    "32x64_w61": (32, 64, "2016-01-01T00", 5844, dict(window_days=61), 3, 48),
    "721x1440_w3": (721, 1440, "2020-03-01T00", 32, dict(window_days=3, days=[63, 64]), 10, 8),
}


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def composed(x, ptr, rows, levels, slots, out):
    """out[:, k] for k < slots from ATen ops; x [T, F, H, W] float32, rows and levels (double) on the device, ptr on
    the host"""
    import torch
    nan = float("nan")
    for k in range(slots):
        a, b = int(ptr[k]), int(ptr[k + 1])
        if a == b:
            out[:, k] = nan
            continue
        v = x.index_select(0, rows[a:b])
        v = torch.where(torch.isfinite(v), v + 0.0, torch.full_like(v, nan))
        s = torch.sort(v, dim=0).values                                  # NaN last
        m = torch.isfinite(s).sum(0, keepdim=True)                       # [1, F, H, W]
        top = (m - 1).clamp(min=0)
        for i in range(levels.numel()):
            pos = levels[i] * top.double()
            lo = pos.floor()
            frac = pos - lo
            lo = lo.long()
            hi = torch.minimum(lo + 1, top)
            vl, vh = s.gather(0, lo).double(), s.gather(0, hi).double()
            o = (vl + (vh - vl) * frac).float()
            out[i, k] = torch.where(m > 0, o, torch.full_like(o, nan))[0]
    return out


def measure(name, packing, rounds):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("quantile_latency.py needs the GPU")
    from paradis_model_amd import _lib
    from paradis_model_amd.climatology import ClimPlan, clim_mean, clim_quantile
    from paradis_model_amd.dataset import DeviceStore
    H, W, first, T, plan_kw, iters, ref_slots = CONFIGS[name]
    dev = torch.device("cuda", 0)
    times = (np.datetime64(first, "h") + 6 * np.arange(T).astype("timedelta64[h]")).astype("datetime64[us]")
    feats = [f"f{j}" for j in range(F - 1)] + ["total_precipitation_6hr"]
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(T, F, H, W, device=dev, generator=g) * 3.0 + 250.0
    x[:, F - 1] = (x[:, F - 1] - 250.0).abs() * 1e-3
    x[:, F - 1][x[:, F - 1] < 2.5e-3] = 0.0                  # precipitation: about 60 % of the cells dry
    x[::7, :, 0, 0] = float("nan")
    stats = {k: np.ones(F, np.float32) for k in ("mean", "std", "min", "max")}
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    store = DeviceStore(x, times, feats, stats, lat, (360.0 / W) * np.arange(W), np.zeros((H, W, 1), np.float32),
                        toa_mean=0.0, toa_std=1.0, device=dev, packing=packing)
    del x
    plan = ClimPlan(store.times_us, **plan_kw)
    K, P, Q = plan.n_slots, H * W, len(LEVELS)
    ptr_h, rows_h, w_h = plan.lists()
    N, longest = int(rows_h.size), int(plan.entries.max())
    ptr, rows, w = (torch.from_numpy(a).to(dev) for a in (ptr_h, rows_h, w_h))
    cols = torch.arange(F, dtype=torch.int32, device=dev)
    out = torch.empty(Q, K, F, H, W, device=dev)
    mean_out = torch.empty(K, F, H, W, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = float(N) * F * P * (4 if packing is None else 2) + 4.0 * Q * K * F * P
    copy_bytes = min(nbytes, float(COPY_CAP))             # (a long list re-reads a small store: the copy need not be as long)
    n_copy = int(copy_bytes // 8)
    src, dst = torch.randn(n_copy, device=dev), torch.empty(n_copy, device=dev)
    decoded = store.rows(0, T)
    ref_slots = min(ref_slots, K)
    ref_out = torch.empty(Q, ref_slots, F, H, W, device=dev)
    lev = torch.tensor(LEVELS, dtype=torch.float64, device=dev)
    fns = {"kernel": (lambda: clim_quantile(store, ptr, rows, cols, LEVELS, max_entries=longest, out=out, flag=flag),
                      iters),
           "copy": (lambda: dst.copy_(src), iters),
           "mean": (lambda: clim_mean(store, ptr, rows, w, cols, mean_out, flag), iters),
           "composed": (lambda: composed(decoded, ptr_h, rows, lev, ref_slots, ref_out), 1)}
    with torch.no_grad():
        for fn, _ in fns.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, n) in fns.items():
                ms[k].append(event_ms(fn, n))
        a, b = out[:, :ref_slots], ref_out
        both = torch.isfinite(a) & torch.isfinite(b)
        agree = {"nan_pattern_equal": bool(torch.equal(torch.isnan(a), torch.isnan(b))),
                 "bits_equal_fraction": float((a.view(torch.int32) == b.view(torch.int32))[both].double().mean().item())
                 if bool(both.any()) else None,
                 "max_rel": float(((a - b).abs()[both].max() / b.abs()[both].max()).item()) if bool(both.any()) else None,
                 "flag": int(flag.item())}
    med = {k: statistics.median(v) for k, v in ms.items()}
    cells = int(_lib.lib.paradis_clim_quantile_cells(longest))
    return {"device": torch.cuda.get_device_name(0), "case": name, "packing": packing or "float32", "grid": f"{H}x{W}",
            "T": T, "F": F, "levels": LEVELS, "slots": K, "entries": N, "entries_per_slot_max": longest,
            "cells_per_workgroup": cells, "store_MB": round(store.nbytes / 1e6, 1),
            "algorithmic_MB": round(nbytes / 1e6, 1), "iters": iters, "rounds": rounds, "ms": round(med["kernel"], 4),
            "ms_all": [round(v, 4) for v in ms["kernel"]], "GBps": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
            "copy_MB": round(copy_bytes / 1e6, 1), "copy_ms": round(med["copy"], 4),
            "copy_ms_all": [round(v, 4) for v in ms["copy"]],
            "copy_GBps": round(copy_bytes / (med["copy"] * 1e-3) / 1e9, 1),
            "fraction_of_copy_rate": round((nbytes / med["kernel"]) / (copy_bytes / med["copy"]), 4),
            "mean_ms": round(med["mean"], 4), "mean_ms_all": [round(v, 4) for v in ms["mean"]],
            "quantile_over_mean": round(med["kernel"] / med["mean"], 2),
            "composed_slots": ref_slots, "composed_ms_per_slot": round(med["composed"] / ref_slots, 4),
            "ms_per_slot": round(med["kernel"] / K, 5),
            "composed_over_fused_per_slot": round((med["composed"] / ref_slots) / (med["kernel"] / K), 1),
            "agreement": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each case's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_latency.json"))
    ap.add_argument("--one", default="", help="(internal) name,packing: measure one case, print JSON")
    a = ap.parse_args()
    if a.one:
        name, packing = a.one.split(",")
        print("RESULT " + json.dumps(measure(name, None if packing == "float32" else packing, a.rounds)), flush=True)
        return
    res = {"tool": "quantile_latency", "cases": []}
    for name in CONFIGS:
        for packing in ("float32", "u16"):
            tag = f"{name},{packing}"
            cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", tag]
            try:
                out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"quantile_latency: {tag} ran out of its {a.limit} s; stopping")
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"quantile_latency: {tag} ended with {out.returncode}; stopping")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res["cases"].append(json.loads(line[len("RESULT "):]))
            print(line, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
