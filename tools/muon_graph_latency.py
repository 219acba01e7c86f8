"""What the HIP graph buys a NorMuon training step, and what a per-step learning-rate push costs it, on the MI355X.

Default model at 32x64, S = 1, fp32 and bf16-mixed, B in {1, 4, 32}.  Per configuration, alternated round by round in one
process:

(a) ``eager`` / ``graph``: the NorMuon step eagerly and as a HIP-graph replay (``harness.GraphedTrainStep``), constant
    learning rate: host time to enqueue a step (nothing waits for the device inside) and device-synchronised wall time
    per step.
(b) under the warm-up of the shipped schedule (300,000 steps, warm-up 1,000: the rate changes on every step), graphed
    AdamW and graphed NorMuon: ``*_push`` sets ``group["lr"]`` and calls ``sync_device_state()`` before every replay
    (a blocking host-to-device copy: the only route before the device schedule existed), ``*_sched`` lets the captured
    ``paradis_lr_schedule`` launch read the table (``schedule.DeviceSchedule``).

One JSON line, also written to profiles/muon_graph_latency.json.  No thresholds: a measurement.

    python tools/muon_graph_latency.py [--rounds 5] [--steps 10] [--batches 1,4,32] [--precisions fp32,amp]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, S = 32, 64, 1
TOTAL, WARMUP, DECAY = 300000, 1000, 0.2


def build(optimizer, graphed, amp, batch, schedule):
    from paradis_model_amd.config import default_config, feature_layout, stub_datamodule
    from paradis_model_amd.harness import GraphedTrainStep, TrainStep, make_grids
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = default_config()
    cfg.training.optimizer.name = optimizer
    lat, lg, og = make_grids(H, W, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda()
    lay = feature_layout(cfg)
    step = TrainStep(model, build_loss(cfg, lat).cuda(), cfg, num_common=lay.num_common_features,
                     n_inputs=cfg.dataset.n_time_inputs, capturable=graphed, amp=amp, schedule=schedule)
    fn = GraphedTrainStep(step, batch, warmup=2) if graphed else step
    return step, fn


def configuration(B, amp, rounds, steps):
    from paradis_model_amd.harness import synthetic_batch
    from paradis_model_amd.schedule import DeviceSchedule, wsd_lambda
    batch = synthetic_batch(H, W, False, B, S, seed=1234, device="cuda")
    wsd = (wsd_lambda(TOTAL, WARMUP, DECAY), TOTAL)
    runs = {}
    for name, optimizer, graphed, schedule in (("eager", "normuon", False, None), ("graph", "normuon", True, None),
                                               ("normuon_push", "normuon", True, None),
                                               ("normuon_sched", "normuon", True, wsd),
                                               ("adamw_push", "adamw", True, None), ("adamw_sched", "adamw", True, wsd)):
        step, fn = build(optimizer, graphed, amp, batch, schedule)
        table = DeviceSchedule(step.opt, *wsd) if name.endswith("_push") else None
        runs[name] = [step, fn, table, 2 if graphed else 0]          # (index of the next step: behind the two warm-up steps)

    def one(name):
        step, fn, table, k = runs[name]
        if table is not None:
            for gi, group in enumerate(step.opt.param_groups):
                group["lr"] = table.host_lr(gi, k)
            step.opt.sync_device_state()
        fn(batch)
        runs[name][3] = k + 1

    for name in runs:
        for _ in range(3):
            one(name)
    torch.cuda.synchronize()
    host, wall = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(rounds):
        for name in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one(name)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[name].append(1e3 * (t1 - t0) / steps)
            wall[name].append(1e3 * (t2 - t0) / steps)
    med = statistics.median
    res = {"B": B, "precision": "bf16-mixed" if amp else "fp32"}
    for name in runs:
        res[name] = {"host_ms": round(med(host[name]), 3), "wall_ms": round(med(wall[name]), 3),
                     "wall_ms_all": [round(v, 3) for v in wall[name]]}
    # the learning rates the two routes ended on (they walked the same table)
    res["lr_end"] = {name: [g["lr"] for g in runs[name][0].opt.param_groups] for name in runs if "_" in name}
    runs.clear()
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="1,4,32")
    ap.add_argument("--precisions", default="fp32,amp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "muon_graph_latency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("muon_graph_latency.py needs the GPU")
    from paradis_model_amd import ops
    res = {"tool": "muon_graph_latency", "device": torch.cuda.get_device_name(0), "gemm": ops.gemm_scheme_name(),
           "model": "default", "grid": f"{H}x{W}", "S": S, "optimizer": "normuon", "rounds": a.rounds,
           "steps_per_round": a.steps, "schedule": {"total": TOTAL, "warmup": WARMUP, "decay": DECAY}, "configurations": []}
    for prec in a.precisions.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            res["configurations"].append(configuration(B, prec == "amp", a.rounds, a.steps))
            print(json.dumps(res["configurations"][-1]), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
