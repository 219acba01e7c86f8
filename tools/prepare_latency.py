"""Store-preparation throughput on the MI355X (paradis_model_amd/prepare.py, csrc/prepare.hip).

The statistics pass (``paradis_store_stats``: field alone, field + one stride's tendency) and the wind launch
(``paradis_cartesian_winds``, every level and the 10 m winds, in place) at 32x64 with T = 1024 (a store past the
256 MiB Infinity Cache) and at 721x1440 with T = 8, default feature list - HIP-event time per call, each against two
references on the same device, alternated in one process:
  copy      an ATen ``copy_`` that moves the same algorithmic bytes (half of them read, half written)
  composed  the same results from ATen ops: ``nanmean``, ``nansum`` of squares, ``amin / amax`` of a NaN-masked copy
            (and the same of ``x[1:] - x[:-1]``); the wind formula in torch (float64 from the float32 fields)
GB/s are algorithmic bytes over time: 4 B per value for the field alone; 8 B with a tendency - two operands per pair,
the bytes a pass of any stride consumes, although with stride 1 the kernel keeps the earlier row in registers and HBM
sees each value once: that rate is operands consumed, not HBM traffic -; 28 B per cell and level + 20 B for the surface
row.

Every configuration runs in a child process of its own under its own time limit; after a child that failed or ran out
of time nothing more is started.  One JSON line, also written to profiles/prepare_latency.json.  No thresholds.

    python tools/prepare_latency.py [--rounds 5] [--limit 240]
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

# (H, W, T, iterations per round of the kernels, of the composed references)
CONFIGS = [(32, 64, 1024, 100, 5), (721, 1440, 8, 30, 3)]


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def composed_stats(x, tendency):
    import torch
    dims = (0, 2, 3)

    def five(v):
        nan = torch.isnan(v)
        n = (~nan).sum(dim=dims)
        mean = torch.nanmean(v.double(), dim=dims)
        sq = torch.nansum(v.double() ** 2, dim=dims)
        lo = torch.where(nan, torch.inf, v).amin(dim=dims)
        hi = torch.where(nan, -torch.inf, v).amax(dim=dims)
        return n, mean, torch.sqrt((sq / n - mean * mean).clamp_min(0.0)), lo, hi
    out = five(x)
    return out + five(x[1:] - x[:-1]) if tendency else out


def composed_winds(t, rows, trig, H, W):
    import torch
    sla, cla = trig[:H].view(H, 1), trig[H:2 * H].view(H, 1)
    slo, clo = trig[2 * H:2 * H + W].view(1, W), trig[2 * H + W:].view(1, W)
    for r in rows:
        u, v = t[:, r["src_u"]].double(), t[:, r["src_v"]].double()
        x = -u * slo - v * sla * clo
        y = u * clo - v * sla * slo
        z = v * cla
        if r["src_w"] >= 0:
            k = ((t[:, r["src_w"]] * 287.05) * t[:, r["src_t"]]).double() / (float(r["level_hpa"]) * 100 * 9.80616)
            x, y, z = x - k * cla * clo, y - k * cla * slo, z - k * sla
        t[:, r["dst_x"]], t[:, r["dst_y"]], t[:, r["dst_z"]] = x.float(), y.float(), z.float()
    return t


def measure(H, W, T, iters, iters_ref, rounds):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prepare_latency.py needs the GPU")
    from paradis_model_amd.config import default_config
    from paradis_model_amd._lib import check, dptr, lib, stream_ptr
    from paradis_model_amd.prepare import StoreStats, WindPlan, cartesian_winds
    dev = torch.device("cuda", 0)
    cfg = default_config()
    levels = list(cfg.features.pressure_levels)
    names = [f"{v}_h{l}" for l in levels for v in ("u_component_of_wind", "v_component_of_wind", "vertical_velocity",
                                                    "temperature", "wind_x", "wind_y", "wind_z")]
    names += ["10m_u_component_of_wind", "10m_v_component_of_wind", "wind_x_10m", "wind_y_10m", "wind_z_10m"]
    F = len(names)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(T, F, H, W, device=dev, generator=g) * 3.0 + 250.0
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    lon = (360.0 / W) * np.arange(W)
    plan = WindPlan(names, names, levels)
    trig, _, _ = plan.trig_tables(lat, lon, dev)
    n_values = x.numel()
    wind_bytes = float(T * H * W * (28 * len(levels) + 20))
    bytes_of = {"stats": 4.0 * n_values, "stats_tend": 8.0 * n_values, "winds": wind_bytes}
    copies = {}
    for key, b in bytes_of.items():                       # a copy_ that moves b bytes: b / 8 floats read, b / 8 written
        n = int(b // 8)
        copies[key] = (torch.randn(n, device=dev), torch.empty(n, device=dev))

    def stats(tendency):
        """the pass alone, by the C entry point: StoreStats.update also keeps the last rows for the next slab"""
        st = StoreStats(F, H, W, (1,) if tendency else (), device=dev)
        acc = st._accumulator()
        ws = torch.empty(lib.paradis_store_stats_ws_bytes(T, F, H, W), dtype=torch.uint8, device=dev)
        return lambda: check(lib.paradis_store_stats(dptr(x), T, None, 0, F, H, W, 0, 1 if tendency else -1, 1, dptr(acc),
                                                     st.n_sets, dptr(ws), stream_ptr()), "store_stats")
    fns = {"stats": (stats(False), iters), "stats_tend": (stats(True), iters),
           "winds": (lambda: cartesian_winds(x, x, plan, lat, lon), iters),
           "copy_stats": (lambda: copies["stats"][1].copy_(copies["stats"][0]), iters),
           "copy_stats_tend": (lambda: copies["stats_tend"][1].copy_(copies["stats_tend"][0]), iters),
           "copy_winds": (lambda: copies["winds"][1].copy_(copies["winds"][0]), iters),
           "composed_stats": (lambda: composed_stats(x, False), iters_ref),
           "composed_stats_tend": (lambda: composed_stats(x, True), iters_ref),
           "composed_winds": (lambda: composed_winds(x, plan.rows, trig, H, W), iters_ref)}
    with torch.no_grad():
        for fn, _ in fns.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, (fn, n) in fns.items():
                ms[name].append(event_ms(fn, n))
        # the two ways agree: statistics of one pass each, winds from the same fields
        st = StoreStats(F, H, W, (1,), device=dev)
        st.update(x)
        got = st.result()
        ref = [v.cpu().numpy() for v in composed_stats(x, True)]
        rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))      # noqa: E731
        agree = {"mean_rel": rel(got["mean"], ref[1]), "std_rel": rel(got["std"], ref[2]),
                 "min_equal": bool(np.array_equal(got["min"], ref[3])), "max_equal": bool(np.array_equal(got["max"], ref[4])),
                 "tendency_std_rel": rel(got["tendencies"][1]["tendency_std"], ref[7]),
                 "count_equal": bool(np.array_equal(got["count"], ref[0]))}
        y0 = x.clone()
        fused = cartesian_winds(y0, y0, plan, lat, lon)
        comp = composed_winds(x.clone(), plan.rows, trig, H, W)
        agree["winds_max_abs_diff"] = float((fused - comp).abs().max())
        agree["winds_equal_fraction"] = float((fused == comp).float().mean())
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "T": T, "F": F, "levels": len(levels),
           "store_GB": round(n_values * 4 / 1e9, 3), "iters": iters, "iters_composed": iters_ref, "rounds": rounds,
           "agreement": agree}
    for key, b in bytes_of.items():
        out[key] = {"algorithmic_MB": round(b / 1e6, 2), "ms": round(med[key], 5),
                    "GBps": round(b / (med[key] * 1e-3) / 1e9, 1),
                    "copy_ms": round(med["copy_" + key], 5), "copy_GBps": round(b / (med["copy_" + key] * 1e-3) / 1e9, 1),
                    "fraction_of_copy_rate": round(med["copy_" + key] / med[key], 3),
                    "composed_ms": round(med["composed_" + key], 5),
                    "composed_over_fused": round(med["composed_" + key] / med[key], 2),
                    "ms_all": [round(v, 5) for v in ms[key]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_latency.json"))
    ap.add_argument("--one", default="", help="(internal) H,W,T,iters,iters_ref: measure one configuration, print JSON")
    a = ap.parse_args()
    if a.one:
        H, W, T, iters, iters_ref = (int(v) for v in a.one.split(","))
        print("RESULT " + json.dumps(measure(H, W, T, iters, iters_ref, a.rounds)), flush=True)
        return
    res = {"tool": "prepare_latency", "configs": []}
    for cfg in CONFIGS:
        tag = "x".join(str(v) for v in cfg[:3])
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", ",".join(str(v) for v in cfg)]
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"prepare_latency: {tag} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"prepare_latency: {tag} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["configs"].append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
