"""Validation latency on the MI355X.

(a) The score launch pair ``validate.score`` against the same numbers composed from what the package offered before it:
``val_loss(out, tgt)`` + ``per_channel_loss`` weighted and unweighted + the report formula of the reference's
``_get_report_rmse`` as ATen ops on the device - HIP-event time per call, the two alternated in one process, at 32x64
with B = 32 and at one 721x1440 state (C = 97).  The score's algorithmic bytes (8 B C H W) over its time is given as a
fraction of the 6.29 TB/s copy rate measured on this device.
(b) ``validate.Validator.step`` per validation step, HIP-graph loop against eager loop, alternated: host time (until
``step`` returns; nothing waits for the device inside) and device-synchronised wall time, for the reduced and the
default model at 32x64.

One JSON line, also written to profiles/val_latency.json.  No thresholds: a measurement.

    python tools/val_latency.py [--rounds 5] [--steps 4] [--batch 4] [--big-grid 721x1440]
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

COPY_TBPS = 6.29
REPORTS = ["geopotential_h500", "specific_humidity_h850", "2m_temperature"]
Q_MIN, Q_MAX = 1e-7, 0.025


def lat_deg(nlat, poles):
    lat = np.linspace(-90.0, 90.0, nlat) if poles else -90.0 + 90.0 / nlat + (180.0 / nlat) * np.arange(nlat)
    return torch.from_numpy(lat.astype(np.float32))


def make_spec():
    from paradis_model_amd.validate import ReportSpec
    return ReportSpec.from_features(REPORTS, report_std=[550.0, 1.0, 12.0], custom_normalization=True, q_min=Q_MIN,
                                    q_max=Q_MAX)


def composed_score(out, tgt, loss, spec, row):
    """the same row from ParadisLoss and torch (reference trainer.py:291-315 for the reports)"""
    C = out.shape[1]
    row[0] = loss(out, tgt)
    row[1:1 + C] = loss.per_channel_loss(out, tgt, weighted=True)
    row[1 + C:1 + 2 * C] = loss.per_channel_loss(out, tgt, weighted=False)
    lw = loss.lat_weights_buf.view(1, -1, 1)
    lmin, lmax = torch.log(torch.tensor(Q_MIN, device=out.device)), torch.log(torch.tensor(Q_MAX, device=out.device))
    for r in range(spec.num_reports):
        c = int(spec.chan[r])
        if spec.cls[r] == 2:
            o, p = (torch.clip(torch.exp(t[:, c] * (lmax - lmin) + lmin) - 1e-12, min=0, max=Q_MAX) for t in (out, tgt))
            err = torch.mean((o - p) ** 2 * lw)
        elif spec.cls[r] == 3:
            o, p = (torch.clip(torch.exp(t[:, c] - 10) - 1e-6, min=0) for t in (out, tgt))
            err = torch.mean((o - p) ** 2 * lw)
        else:
            err = torch.mean(((out[:, c] - tgt[:, c]) * float(spec.p1[r])) ** 2 * lw)
        row[1 + 2 * C + r] = torch.sqrt(err)


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def score_times(B, H, W, poles, rounds, iters):
    from paradis_model_amd.config import default_config
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.validate import row_size, score
    loss = build_loss(default_config(), lat_deg(H, poles)).cuda()
    spec = make_spec()
    C = loss.num_features
    g = torch.Generator(device="cuda").manual_seed(11)
    true = torch.randn(B, 2, C, H, W, device="cuda", generator=g)
    true[:, :, int(spec.chan[1])].uniform_(0.0, 1.0, generator=g)
    tgt = true[:, 1]                                  # a view with batch stride S*C*H*W, as in the validation loop
    out = tgt + 0.3 * torch.randn(B, C, H, W, device="cuda", generator=g)
    a, b = (torch.zeros(row_size(C, spec.num_reports), device="cuda") for _ in range(2))
    fns = {"score": lambda: score(out, tgt, loss, spec, a), "composed": lambda: composed_score(out, tgt, loss, spec, b)}
    with torch.no_grad():
        for fn in fns.values():                       # warm-up of both, this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ms[k].append(event_ms(fn, iters))
    nbytes = 8.0 * B * C * H * W
    t = statistics.median(ms["score"])
    rate = nbytes / (t * 1e-3) / 1e12
    return {"grid": f"{H}x{W}", "B": B, "C": C, "reports": REPORTS, "loss": loss.kind, "iters": iters, "rounds": rounds,
            "score_ms": round(t, 5), "composed_ms": round(statistics.median(ms["composed"]), 5),
            "score_ms_all": [round(v, 5) for v in ms["score"]], "composed_ms_all": [round(v, 5) for v in ms["composed"]],
            "algorithmic_MB": round(nbytes / 1e6, 2), "score_TBps": round(rate, 3),
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3),
            "score_vs_composed_max_rel": float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())}


def step_times(which, B, S, rounds):
    from paradis_model_amd.config import default_config, reduced_config, stub_datamodule
    from paradis_model_amd.harness import make_grids, synthetic_batch
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    from paradis_model_amd.validate import Validator
    cfg = default_config() if which == "default" else reduced_config()
    H, W = 32, 64
    lat, lg, og = make_grids(H, W, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda().eval()
    loss = build_loss(cfg, lat).cuda()
    batch = synthetic_batch(H, W, False, B, S, device="cuda")
    vals = {g: Validator(model, loss, make_spec(), graph=g) for g in (False, True)}
    for g in (False, True):                           # warm-up (and the capture)
        vals[g].step(batch)
        vals[g].step(batch)
    torch.cuda.synchronize()
    host, dev = {False: [], True: []}, {False: [], True: []}
    for _ in range(rounds):
        for g in (False, True):
            t0 = time.perf_counter()
            vals[g].step(batch)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[g].append(1e3 * (t1 - t0) / S)
            dev[g].append(1e3 * (t2 - t0) / S)
    med = statistics.median
    res = vals[True].result()
    return {"model": which, "grid": f"{H}x{W}", "B": B, "steps": S, "rounds": rounds,
            "eager_host_ms_per_step": round(med(host[False]), 3), "graph_host_ms_per_step": round(med(host[True]), 3),
            "eager_device_ms_per_step": round(med(dev[False]), 3), "graph_device_ms_per_step": round(med(dev[True]), 3),
            "eager_device_ms_all": [round(v, 3) for v in dev[False]], "graph_device_ms_all": [round(v, 3) for v in dev[True]],
            "val_loss": res["val_loss"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--big-grid", default="721x1440", help="one state of this grid for the score times ('' to skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_latency.py needs the GPU")
    from paradis_model_amd import ops
    res = {"tool": "val_latency", "device": torch.cuda.get_device_name(0), "gemm": ops.gemm_scheme_name(),
           "copy_rate_TBps": COPY_TBPS, "score": [], "step": []}
    res["score"].append(score_times(32, 32, 64, False, a.rounds, 2000))
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        res["score"].append(score_times(1, H, W, H % 2 == 1, a.rounds, 200))
    for which in ("reduced", "default"):
        res["step"].append(step_times(which, a.batch, a.steps, a.rounds))
    line = json.dumps(res)
    print(line, flush=True)
    out = os.path.join(ROOT, "profiles", "val_latency.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
