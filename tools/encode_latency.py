"""Forecast-encoding latency on the MI355X.

``encode.encode_chunk`` (one launch of ``csrc/encode.hip``: the writer's variables regrouped out of a chunk and passed
through BitRound) against two baselines on the same device - the same result composed from ATen ops (``index_select``
per variable, ``cat``, integer ops on a ``view(torch.int32)``) and an ATen ``copy_`` of the same number of bytes - HIP-event
time per call, the three alternated in one process, at 32x64 with B = 32 and at one 721x1440 state, C = 97, L = 13,
keepbits 16.  The launch's algorithmic bytes (8 per encoded value) over its time is given as a fraction of the 6.29 TB/s
copy rate measured on this device.

Then a whole flush - what ``Forecaster.run`` enqueues when a chunk is full - with the encoder (the launch, then one
device-to-host copy of the 96 encoded planes per state into pinned memory) against today's (device-to-host copies of
the 97-channel chunk and the 13-level dew-point chunk), timed from the host around a synchronisation.

Every timed configuration runs in a child process of its own under its own time limit; after a child that failed or ran
out of time nothing more is started.

One JSON line, also written to profiles/encode_latency.json.  No thresholds: a measurement.

    python tools/encode_latency.py [--rounds 5] [--big-grid 721x1440] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29
KEEPBITS = 16


def make_composed(spec, chunk, dew):
    """the encoded buffer from ATen ops (what a user composes on the device without the kernel)"""
    import torch
    idx = [torch.tensor([s if s >= 0 else -1 - s for s in v.sources], device=chunk.device) for v in spec.variables]
    from_dew = [v.sources[0] < 0 for v in spec.variables]
    m = 23 - KEEPBITS
    half, mask = (1 << (m - 1)) - 1, -(1 << m)

    def run():
        parts = [(dew if d else chunk).index_select(2, i).reshape(-1) for i, d in zip(idx, from_dew)]
        b = torch.cat(parts).view(torch.int32)
        b = (b + (((b >> m) & 1) + half)) & mask
        return b.view(torch.float32)
    return run


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def host_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def measure(B, H, W, rounds, iters):
    import torch
    from paradis_model_amd.config import default_config, feature_layout
    from paradis_model_amd.encode import EncodeSpec, encode_chunk
    if not torch.cuda.is_available():
        raise SystemExit("encode_latency.py needs the GPU")
    cfg = default_config()
    names = feature_layout(cfg).output_name_order
    spec = EncodeSpec.from_config(cfg, names, cfg.features.pressure_levels, keepbits=KEEPBITS)
    C, L, n = spec.num_channels, spec.num_levels, 1
    g = torch.Generator(device="cuda").manual_seed(11)
    chunk = torch.randn(B, n, C, H, W, device="cuda", generator=g) * 40
    dew = torch.rand(B, n, L, H, W, device="cuda", generator=g) * 30
    numel = spec.numel(B, n, H, W)
    out = torch.empty(numel, device="cuda")
    src, dst = torch.randn(numel, device="cuda", generator=g), torch.empty(numel, device="cuda")
    composed = make_composed(spec, chunk, dew)
    fns = {"encode": lambda: encode_chunk(chunk, dew, spec, out, n, 0), "composed": composed,
           "copy": lambda: dst.copy_(src)}
    # the two flushes: pinned buffers as Forecaster.run holds them
    henc = torch.empty(numel, pin_memory=True)
    h, dh = torch.empty(B, n, C, H, W, pin_memory=True), torch.empty(B, n, L, H, W, pin_memory=True)

    def flush_encoded():
        encode_chunk(chunk, dew, spec, out, n, 0)
        henc.copy_(out, non_blocking=True)

    def flush_plain():
        h.copy_(chunk, non_blocking=True)
        dh.copy_(dew, non_blocking=True)

    flushes = {"flush_encoded": flush_encoded, "flush_plain": flush_plain}
    with torch.no_grad():
        for fn in list(fns.values()) + list(flushes.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in list(fns) + list(flushes)}
        for _ in range(rounds):
            for name, fn in fns.items():
                ms[name].append(event_ms(fn, iters))
            for name, fn in flushes.items():
                ms[name].append(host_ms(fn, max(3, iters // 20)))
        encode_chunk(chunk, dew, spec, out, n, 0)
        same = bool(torch.equal(out.view(torch.int32), composed().view(torch.int32)))
    nbytes = 8.0 * numel
    med = {k: statistics.median(v) for k, v in ms.items()}
    rate = nbytes / (med["encode"] * 1e-3) / 1e12
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "B": B, "n": n, "C": C, "planes": spec.n_planes,
            "keepbits": KEEPBITS, "iters": iters, "rounds": rounds,
            "encode_ms": round(med["encode"], 5), "composed_ms": round(med["composed"], 5),
            "copy_ms": round(med["copy"], 5), "flush_encoded_ms": round(med["flush_encoded"], 4),
            "flush_plain_ms": round(med["flush_plain"], 4),
            "all_ms": {k: [round(x, 5) for x in v] for k, v in ms.items()},
            "algorithmic_MB": round(nbytes / 1e6, 2), "encode_TBps": round(rate, 3),
            "fraction_of_copy_rate": round(rate / COPY_TBPS, 3),
            "copy_TBps": round(nbytes / (med["copy"] * 1e-3) / 1e12, 3),
            "flush_encoded_MB": round(4.0 * numel / 1e6, 2), "flush_plain_MB": round(4.0 * (chunk.numel() + dew.numel()) / 1e6, 2),
            "encode_equals_composed_bit_for_bit": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-grid", default="721x1440", help="one state of this grid ('' to skip)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_latency.json"))
    ap.add_argument("--one", default="", help="(internal) B,H,W,iters: measure one configuration, print JSON")
    a = ap.parse_args()
    if a.one:
        B, H, W, iters = (int(v) for v in a.one.split(","))
        print("RESULT " + json.dumps(measure(B, H, W, a.rounds, iters)), flush=True)
        return
    configs = [(32, 32, 64, 1000)]
    if a.big_grid:
        H, W = (int(v) for v in a.big_grid.split("x"))
        configs.append((1, H, W, 200))
    res = {"tool": "encode_latency", "copy_rate_TBps": COPY_TBPS, "encode": []}
    for (B, H, W, iters) in configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", f"{B},{H},{W},{iters}"]
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"encode_latency: B={B} {H}x{W} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"encode_latency: B={B} {H}x{W} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["encode"].append(json.loads(line[len("RESULT "):]))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
