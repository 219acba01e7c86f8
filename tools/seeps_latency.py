"""SEEPS latency on the MI355X: the climatology launch (paradis_model_amd/climatology.py ``clim_seeps``, csrc/quantile.hip
``paradis_clim_seeps`` / ``paradis_clim_seeps_packed``) and the table update (``seeps.SeepsTable.update``,
csrc/seeps.hip).

Climatology: the three configurations, stores and lists of tools/quantile_latency.py (F = 9 features, float32 and
``packing="u16"``, every feature a column of the launch so that the bytes read are those of that tool's cases), dry
threshold 2.5e-3, against, alternated in one process,
  copy      an ATen ``copy_`` that moves the same algorithmic bytes (half read, half written), 2 GiB at the most
  quantile  ``clim_quantile`` with ONE level on the same lists: the same fill and sort, the other stage behind them
  composed  the same two planes from ATen ops, slot by slot: ``index_select``, non-finite to NaN, ``sort`` (NaN last),
            the counts of kept and of dry values, two ``gather``s and the lerp in double; over the first slots only,
            reported per slot.
Update: one precipitation channel of a 4-channel state at 721x1440 B = 1 and at 32x64 B = 32, K = 4 slots, against
  copy      an ATen ``copy_`` of as many bytes as the launches read (16 per cell)
  composed  the same counters and row sums from ATen ops: comparisons for the categories, the matrix entry by
            ``torch.where`` in double, ``bincount`` for the table.  Its integers must equal the kernel's
            (``ints_equal``); its sums agree to the rounding of another summation order (``sums_max_rel``).
HIP-event time per call.  GB/s are algorithmic bytes over time.

Every case runs in a child process of its own under its own time limit; after a child that failed or ran out of time
nothing more is started.  One JSON line, also written to profiles/seeps_latency.json.  No thresholds: a measurement.

    python tools/seeps_latency.py [--rounds 5] [--limit 240]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from quantile_latency import CONFIGS, COPY_CAP, F, event_ms      # noqa: E402  (the same stores and lists)

DRY = 2.5e-3
WET_LEVEL = 2.0 / 3.0
UPDATES = {"721x1440_B1": (1, 721, 1440, 50, 5), "32x64_B32": (32, 32, 64, 500, 20)}   # B, H, W, iters, iters composed


def composed_clim(x, ptr, rows, slots, out):
    """out[:, k] for k < slots from ATen ops; x [T, F, H, W] float32 and rows on the device, ptr on the host"""
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
        n_dry = (s < DRY).sum(0, keepdim=True)
        top = (m - n_dry - 1).clamp(min=0)
        pos = WET_LEVEL * top.double()
        lo = pos.floor()
        frac = pos - lo
        lo = lo.long()
        hi = torch.minimum(lo + 1, top)
        last = (m - 1).clamp(min=0)
        vl = s.gather(0, torch.minimum(n_dry + lo, last)).double()
        vh = s.gather(0, torch.minimum(n_dry + hi, last)).double()
        thr = (vl + (vh - vl) * frac).float()
        out[0, k] = torch.where(m > 0, (n_dry.double() / m.clamp(min=1).double()).float(), torch.full_like(thr, nan))[0]
        out[1, k] = torch.where(m - n_dry > 0, thr, torch.full_like(thr, nan))[0]
    return out


def measure_clim(name, packing, rounds):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seeps_latency.py needs the GPU")
    from paradis_model_amd import _lib
    from paradis_model_amd.climatology import ClimPlan, clim_quantile, clim_seeps
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
    K, P = plan.n_slots, H * W
    ptr_h, rows_h, _ = plan.lists()
    N, longest = int(rows_h.size), int(plan.entries.max())
    ptr, rows = torch.from_numpy(ptr_h).to(dev), torch.from_numpy(rows_h).to(dev)
    cols = torch.arange(F, dtype=torch.int32, device=dev)
    out = torch.empty(2, K, F, H, W, device=dev)
    q_out = torch.empty(1, K, F, H, W, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = float(N) * F * P * (4 if packing is None else 2) + 8.0 * K * F * P
    copy_bytes = min(nbytes, float(COPY_CAP))
    n_copy = int(copy_bytes // 8)
    src, dst = torch.randn(n_copy, device=dev), torch.empty(n_copy, device=dev)
    decoded = store.rows(0, T)
    ref_slots = min(ref_slots, K)
    ref_out = torch.empty(2, ref_slots, F, H, W, device=dev)
    fns = {"kernel": (lambda: clim_seeps(store, ptr, rows, cols, DRY, wet_level=WET_LEVEL, max_entries=longest, out=out,
                                         flag=flag), iters),
           "copy": (lambda: dst.copy_(src), iters),
           "quantile": (lambda: clim_quantile(store, ptr, rows, cols, [WET_LEVEL], max_entries=longest, out=q_out,
                                              flag=flag), iters),
           "composed": (lambda: composed_clim(decoded, ptr_h, rows, ref_slots, ref_out), 1)}
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
                 "flag": int(flag.item())}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"device": torch.cuda.get_device_name(0), "case": name, "packing": packing or "float32", "grid": f"{H}x{W}",
            "T": T, "F": F, "slots": K, "entries": N, "entries_per_slot_max": longest,
            "cells_per_workgroup": int(_lib.lib.paradis_clim_quantile_cells(longest)),
            "algorithmic_MB": round(nbytes / 1e6, 1), "iters": iters, "rounds": rounds, "ms": round(med["kernel"], 4),
            "ms_all": [round(v, 4) for v in ms["kernel"]], "GBps": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
            "copy_MB": round(copy_bytes / 1e6, 1), "copy_ms": round(med["copy"], 4),
            "copy_GBps": round(copy_bytes / (med["copy"] * 1e-3) / 1e9, 1),
            "fraction_of_copy_rate": round((nbytes / med["kernel"]) / (copy_bytes / med["copy"]), 4),
            "quantile_one_level_ms": round(med["quantile"], 4),
            "quantile_one_level_ms_all": [round(v, 4) for v in ms["quantile"]],
            "seeps_over_quantile": round(med["kernel"] / med["quantile"], 3),
            "composed_slots": ref_slots, "composed_ms_per_slot": round(med["composed"] / ref_slots, 4),
            "ms_per_slot": round(med["kernel"] / K, 5),
            "composed_over_fused_per_slot": round((med["composed"] / ref_slots) / (med["kernel"] / K), 1),
            "agreement": agree}


def composed_update(f, o, p1, thr, dry, p_lo, p_hi):
    """(sums double [H, 3], counts int64 [H, 10]) of one channel from ATen ops; f, o, p1, thr [B, H, W] float32"""
    import torch
    B, H, W = f.shape
    fin = torch.isfinite(f) & torch.isfinite(o) & torch.isfinite(p1) & torch.isfinite(thr)
    ok = fin & (p1 >= p_lo) & (p1 <= p_hi)
    cf = torch.where(f < dry, 0, torch.where(f >= thr, 2, 1))
    co = torch.where(o < dry, 0, torch.where(o >= thr, 2, 1))
    p = p1.double()
    a, b, c = 1.0 / (1.0 - p), 1.0 / p, 3.0 / (2.0 + p)
    zero = torch.zeros_like(p)
    m0 = torch.where(co == 0, zero, torch.where(co == 1, a, 4.0 * a))
    m1 = torch.where(co == 0, b, torch.where(co == 1, zero, 3.0 * a))
    m2 = torch.where(co == 0, b + c, torch.where(co == 1, c, zero))
    s = 0.5 * torch.where(cf == 0, m0, torch.where(cf == 1, m1, m2))
    sums = torch.stack([torch.where(ok & (co == j), s, zero).sum(dim=(0, 2)) for j in range(3)], dim=-1)
    row = torch.arange(H, device=f.device).view(1, H, 1).expand(B, H, W)
    cls = torch.where(ok, 3 * cf + co, 9)
    hist = torch.bincount((row * 10 + cls)[fin], minlength=H * 10).view(H, 10)
    return sums, hist


def measure_update(name, rounds):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seeps_latency.py needs the GPU")
    from paradis_model_amd.climatology import SeepsClimatology
    from paradis_model_amd.seeps import SeepsTable
    B, H, W, iters, iters_composed = UPDATES[name]
    C, K = 4, 4
    g = torch.Generator(device="cuda").manual_seed(13)

    def rain(*shape):
        x = torch.randn(*shape, device="cuda", generator=g).abs() * 1e-3
        x[torch.rand(*shape, device="cuda", generator=g) < 0.4] = 0.0
        return x

    f, o = rain(B, C, H, W), rain(B, C, H, W)
    data = torch.empty(2, K, 1, H, W, device="cuda")
    data[0] = 0.02 + 0.96 * torch.rand(K, 1, H, W, device="cuda", generator=g)
    data[1] = 0.5e-3 + 1e-3 * torch.rand(K, 1, H, W, device="cuda", generator=g)
    names = [f"c{i}" for i in range(C - 1)] + ["total_precipitation_6hr"]
    dry = 0.25e-3
    clim = SeepsClimatology(data, None, [names[-1]], dry)
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    table = SeepsTable(names, lat, 1, clim)
    idx = (torch.arange(B, device="cuda") % K).to(torch.int32)
    p_lo, p_hi = table.p1_bounds
    nbytes = 16 * B * H * W
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    args = (f[:, C - 1], o[:, C - 1], data[0, idx.long(), 0], data[1, idx.long(), 0], table.dry_threshold, p_lo, p_hi)
    fns = {"update": (lambda: table.update(0, f, o, idx), iters), "copy": (lambda: dst.copy_(src), iters),
           "composed": (lambda: composed_update(*args), iters_composed)}
    with torch.no_grad():
        for fn, _ in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, n) in fns.items():
                ms[k].append(event_ms(fn, n))
        table.reset()
        table.update(0, f, o, idx)
        sums, ints = composed_update(*args)
        ints_equal = bool(torch.equal(table.acc_int[0, 0], ints))
        rel = ((table.acc_real[0, 0] - sums).abs() / table.acc_real[0, 0].abs().clamp_min(1e-300)).max()
    tm, tc, ta = (statistics.median(ms[n]) for n in ("update", "copy", "composed"))
    return {"device": torch.cuda.get_device_name(0), "case": name, "grid": f"{H}x{W}", "B": B, "channels": 1, "slots": K,
            "iters": iters, "iters_composed": iters_composed, "rounds": rounds, "update_ms": round(tm, 5),
            "copy_ms": round(tc, 5), "composed_ms": round(ta, 5), "update_ms_all": [round(v, 5) for v in ms["update"]],
            "copy_ms_all": [round(v, 5) for v in ms["copy"]], "composed_ms_all": [round(v, 5) for v in ms["composed"]],
            "algorithmic_MB": round(nbytes / 1e6, 3), "update_GBps": round(nbytes / (tm * 1e-3) / 1e9, 1),
            "copy_GBps": round(2 * nbytes / (tc * 1e-3) / 1e9, 1),          # a copy reads and writes its bytes
            "update_over_copy": round(tm / tc, 3), "composed_over_update": round(ta / tm, 1), "ints_equal": ints_equal,
            "sums_max_rel": float(rel)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each case's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeps_latency.json"))
    ap.add_argument("--one", default="", help="(internal) clim,name,packing or update,name: measure one case, print JSON")
    a = ap.parse_args()
    if a.one:
        kind, name, *rest = a.one.split(",")
        res = measure_update(name, a.rounds) if kind == "update" else \
            measure_clim(name, None if rest[0] == "float32" else rest[0], a.rounds)
        print("RESULT " + json.dumps(res), flush=True)
        return
    tags = [f"update,{name}" for name in UPDATES] + [f"clim,{name},{p}" for name in CONFIGS for p in ("float32", "u16")]
    res = {"tool": "seeps_latency", "update": [], "clim": []}
    for tag in tags:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", tag]
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"seeps_latency: {tag} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"seeps_latency: {tag} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res[tag.split(",")[0]].append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
