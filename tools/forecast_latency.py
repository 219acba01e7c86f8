"""Forecast latency on the MI355X (row f5): the predict loop ``forecast.Forecaster`` with the default model at 32x64,
B in {1, 4} - device-synchronised wall time per step of the eager loop and of the HIP-graph loop, the two alternated in
one process - and the HIP-event time of ``forecast.postprocess`` against the same result composed from what the package
offered before it (permute to channels-last, ``feed.normalize_features_(inverse=True)``, permute back, the wind
formulas as float64 torch ops on the device).  One JSON line, also written to profiles/forecast_latency.json.

    python tools/forecast_latency.py [--steps 40] [--rounds 3] [--post-grid 721x1440]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_deg(nlat, nlon, poles):
    lat = np.linspace(-90.0, 90.0, nlat) if poles else -90.0 + 90.0 / nlat + (180.0 / nlat) * np.arange(nlat)
    return lat, np.arange(nlon) * (360.0 / nlon)


def make_spec(dewpoint=True):
    from paradis_model_amd.config import default_config, feature_layout
    from paradis_model_amd.forecast import PostSpec
    cfg = default_config()
    names = feature_layout(cfg).output_name_order
    zs = [n for n in names if not n.startswith("specific_humidity") and n != "total_precipitation_6hr"]
    g = torch.Generator().manual_seed(3)
    mean, std = torch.randn(len(zs), generator=g) * 10, torch.rand(len(zs), generator=g) * 5 + 0.5
    for i, n in enumerate(zs):
        if "temperature" in n:
            mean[i], std[i] = 250.0, 15.0
    return PostSpec.from_features(names, cfg.features.pressure_levels, zscore_mean=mean, zscore_std=std, q_min=1e-7,
                                  q_max=0.025, custom_normalization=True, dewpoint=dewpoint)


def composed_post(x, spec, lat, lon, chunk, slot):
    """the same state from the package's older pieces + torch"""
    from paradis_model_amd import feed
    cl = x.permute(0, 2, 3, 1).contiguous()
    feed.normalize_features_(cl, spec.kind, spec.p0, spec.p1, spec.eps_q, inverse=True)
    y = cl.permute(0, 3, 1, 2).contiguous()
    la = torch.deg2rad(torch.as_tensor(lat, dtype=torch.float64, device=x.device)).view(-1, 1)
    lo = torch.deg2rad(torch.as_tensor(lon, dtype=torch.float64, device=x.device)).view(1, -1)
    sla, cla, slo, clo = torch.sin(la), torch.cos(la), torch.sin(lo), torch.cos(lo)
    X, Y, Z, T = (y[:, i].double() for i in (spec.ix, spec.iy, spec.iz, spec.it))
    p = torch.as_tensor(spec.pressure_levels, dtype=torch.float64, device=x.device).view(-1, 1, 1)
    u = -X * slo + Y * clo
    v = -X * sla * clo - Y * sla * slo + Z * cla
    w = (-X * cla * clo - Y * cla * slo - Z * sla) * (p * 100 * 9.80616 / (287.05 * T))
    y[:, spec.ix], y[:, spec.iy], y[:, spec.iz] = u.float(), v.float(), w.float()
    sx, sy, sz = spec.sfc
    X, Y, Z = (y[:, i].double() for i in (sx, sy, sz))
    y[:, sx], y[:, sy] = (-X * slo + Y * clo).float(), (-X * sla * clo - Y * sla * slo + Z * cla).float()
    chunk[:, slot] = y


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def post_times(B, H, W, poles, iters=20):
    from paradis_model_amd.forecast import postprocess
    from tests._util import max_rel
    spec = make_spec(dewpoint=False)
    lat, lon = grid_deg(H, W, poles)
    C = spec.num_channels
    x = torch.randn(B, C, H, W, device="cuda")
    a, b = torch.zeros(B, 1, C, H, W, device="cuda"), torch.zeros(B, 1, C, H, W, device="cuda")
    fused = event_ms(lambda: postprocess(x, spec, lat, lon, a, 0), iters)
    comp = event_ms(lambda: composed_post(x, spec, lat, lon, b, 0), iters)
    nbytes = 8.0 * B * C * H * W
    return {"grid": f"{H}x{W}", "B": B, "post_fused_ms": round(fused, 4), "post_composed_ms": round(comp, 4),
            "post_algorithmic_MB": round(nbytes / 1e6, 2), "post_fused_GBps": round(nbytes / fused / 1e6, 1),
            "fused_vs_composed_max_rel": max_rel(a, b)}


def rollout_times(B, steps, rounds):
    from paradis_model_amd.config import default_config, stub_datamodule
    from paradis_model_amd.forecast import Forecaster
    from paradis_model_amd.harness import make_grids, synthetic_batch
    from paradis_model_amd.model import Paradis
    cfg = default_config()
    H, W = 32, 64
    _, lg, og = make_grids(H, W, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda().eval()
    inp, _, forc, const = synthetic_batch(H, W, False, B, steps, device="cuda")
    lat, lon = grid_deg(H, W, False)
    spec = make_spec()
    fcs = {g: Forecaster(model, spec, lat, lon, write_every_n=8, graph=g) for g in (False, True)}
    sink = lambda **kw: None       # noqa: E731
    ms = {False: [], True: []}
    for g in (False, True):        # warm-up (and the capture)
        fcs[g].run(inp, forc, const, sink)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for g in (False, True):
            t0 = time.perf_counter()
            fcs[g].run(inp, forc, const, sink)
            torch.cuda.synchronize()
            ms[g].append(1e3 * (time.perf_counter() - t0) / steps)
    return {"grid": f"{H}x{W}", "B": B, "steps": steps, "rounds": rounds,
            "eager_ms_per_step": round(statistics.median(ms[False]), 3),
            "graph_ms_per_step": round(statistics.median(ms[True]), 3),
            "eager_ms_all": [round(v, 3) for v in ms[False]], "graph_ms_all": [round(v, 3) for v in ms[True]]}


def host_times(steps, rounds=7):
    """host time per step of the graphed run with on_chunk=None (nothing synchronised inside the timed call), B = 1,
    every step stored, chunks of 2 - the most hand-over work per step - plain and with an encoder"""
    from paradis_model_amd.config import default_config, stub_datamodule
    from paradis_model_amd.encode import EncodeSpec
    from paradis_model_amd.forecast import Forecaster
    from paradis_model_amd.harness import make_grids, synthetic_batch
    from paradis_model_amd.model import Paradis
    cfg = default_config()
    H, W = 32, 64
    _, lg, og = make_grids(H, W, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda().eval()
    inp, _, forc, const = synthetic_batch(H, W, False, 1, steps, device="cuda")
    lat, lon = grid_deg(H, W, False)
    spec = make_spec()
    enc = EncodeSpec.from_config(cfg, spec.names, list(cfg.features.pressure_levels))
    res = {"grid": f"{H}x{W}", "B": 1, "steps": steps, "write_every_n": 2, "rounds": rounds}
    for name, kw in (("plain", {}), ("encoded", {"encoder": enc})):
        fc = Forecaster(model, spec, lat, lon, write_every_n=2, graph=True)
        fc.run(inp, forc, const, lambda **k: None, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            fc.run(inp, forc, const, None, **kw)
            ms.append(1e3 * (time.perf_counter() - t0) / steps)
            torch.cuda.synchronize()
        res[f"{name}_host_ms_per_step"] = round(statistics.median(ms), 4)
        res[f"{name}_host_ms_all"] = [round(v, 4) for v in ms]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--post-grid", default="721x1440", help="an extra grid for the post-processing times ('' to skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("forecast_latency.py needs the GPU")
    from paradis_model_amd import ops
    res = {"tool": "forecast_latency", "device": torch.cuda.get_device_name(0), "gemm": ops.gemm_scheme_name(),
           "rollout": [], "post": [], "host": host_times(max(40, a.steps))}
    for B in (1, 4):
        res["post"].append(post_times(B, 32, 64, False))
        res["rollout"].append(rollout_times(B, max(40, a.steps), a.rounds))
    if a.post_grid:
        H, W = (int(v) for v in a.post_grid.split("x"))
        res["post"].append(post_times(1, H, W, H % 2 == 1))
    line = json.dumps(res)
    print(line, flush=True)
    out = os.path.join(ROOT, "profiles", "forecast_latency.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
