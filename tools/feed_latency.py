"""Batch-assembly latency of the device-resident dataset on the MI355X.

``dataset.DeviceDataset.batch`` (one launch of ``csrc/feed.hip::paradis_assemble_batch`` for input and target, the
forcings launch, the cached constants) against the same tuple composed on the same device from ATen gathers,
``feed.normalize_features_`` (channels-last, as it is defined) and permutes, with the same forcings call - HIP-event time
per call, the two alternated in one process - at 32x64 with B = 32 (S = 1 and S = 6), 128x256 with B = 8 and one
721x1440 sample, default feature list (97 stored features, 166 input and 97 target planes per step).  The assembly
launch alone is timed too, and a ``copy_`` of as many floats as it writes: the device's copy rate at this size, the
same 8 B per value.  ``fraction_of_copy_rate`` = copy time / assembly time.

The store is sized past the 256 MiB Infinity Cache and every call takes another set of sample indices, so the reads
come from HBM.  Every configuration runs in a child process of its own under its own time limit; after a child that
failed or ran out of time nothing more is started.

``--packing u16`` adds the packed store (``DeviceStore(packing="u16")``) of the same data in the same process, its
calls alternated with the float ones: the packed assembly launch and a whole ``batch()`` from it
(``packed_over_float_assemble`` = packed / float assembly time; by bytes 6 / 8), and on one upload slab
(``dataset.SLAB_BYTES`` of float32 rows) the pack launch, the unpack launch and an ATen ``copy_`` of the slab.

One JSON line, also written to profiles/feed_latency.json (profiles/feed_latency_u16.json with ``--packing``).  No
thresholds: a measurement.

    python tools/feed_latency.py [--rounds 5] [--limit 240] [--packing u16]
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

# (H, W, B, S, store times, iterations per round)
CONFIGS = [(32, 64, 32, 1, 1024, 1000), (32, 64, 32, 6, 1024, 300), (128, 256, 8, 1, 96, 300), (721, 1440, 1, 1, 8, 100)]
N_INDEX_SETS = 16


def build(H, W, T, S):
    """a store of the default feature list with random contents, generated on the device from a seed"""
    import torch
    from paradis_model_amd.config import default_config, feature_layout
    from paradis_model_amd.dataset import DeviceDataset, DeviceStore
    cfg = default_config()
    names = feature_layout(cfg).output_name_order                  # the 97 stored features (inputs are a subset)
    F = len(names)
    g = torch.Generator(device="cuda").manual_seed(3)
    data = torch.rand(T, F, H, W, device="cuda", generator=g) * 0.02 + 1e-4     # positive: every kind is defined
    stats = {"mean": np.full(F, 0.01, np.float32), "std": np.full(F, 0.006, np.float32),
             "min": np.full(F, 1e-7, np.float32), "max": np.full(F, 0.025, np.float32)}
    times = np.datetime64("1979-01-01T00", "us") + np.arange(T) * np.timedelta64(6, "h")
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    lon = (360.0 / W) * np.arange(W)
    constants = torch.randn(H, W, len(cfg.features.input.constants), device="cuda", generator=g)
    store = DeviceStore(data, times, names, stats, lat.astype(np.float32), lon.astype(np.float32), constants, 251.3, 302.7)
    del data
    n_t = cfg.dataset.n_time_inputs
    start = str(times[n_t - 1].astype("datetime64[s]"))
    end = str(times[T - 1 - S].astype("datetime64[s]"))
    ds = DeviceDataset(store, cfg, start, end, S)
    ds.span = (start, end)
    return ds


def packed_twin(ds, packing):
    """the dataset of ``ds`` over a packed store of the same values"""
    from paradis_model_amd.dataset import DeviceDataset, DeviceStore
    st = ds.store
    store = DeviceStore(st.data, st.times_us, st.features, st.stats, st.lat, st.lon, st.constants, st.toa_mean,
                        st.toa_std, device=st.device, packing=packing)
    return DeviceDataset(store, ds.cfg, *ds.span, ds.forecast_steps)


def composed(ds, idx):
    """the batch tuple from ATen gathers + normalize_features_ + permutes (what a user composes without the kernel)"""
    import torch
    from paradis_model_amd import feed
    data, n_t, S = ds.store.data, ds.n_time_inputs, ds.forecast_steps
    t_in = ds.base + idx * ds.interval_steps
    x = torch.cat([data[t_in + k][:, ds._in_cols_dev].permute(0, 2, 3, 1) for k in range(n_t)], dim=-1).contiguous()
    feed.normalize_features_(x, ds._kind_in_dev, ds._p0_in_dev, ds._p1_in_dev)
    inp = x.permute(0, 3, 1, 2).unsqueeze(1).contiguous()
    t_out = t_in + n_t + ds.prediction_shift
    y = torch.stack([data[t_out + s][:, ds._out_cols_dev].permute(0, 2, 3, 1) for s in range(S)], dim=1).contiguous()
    feed.normalize_features_(y, ds._kind_out_dev, ds._p0_out_dev, ds._p1_out_dev)
    tgt = y.permute(0, 1, 4, 2, 3).contiguous()
    rows = t_in.unsqueeze(1) + torch.arange(S + n_t - 1, device=idx.device)
    forc = feed.compute_forcings(ds.store.times_dev[rows], ds.store.lat_dev, ds.store.lon_dev, n_t, ds.store.toa_mean,
                                 ds.store.toa_std, ds.forcing_inputs, device=idx.device)
    H, W, Cc = ds.store.constants.shape
    const = ds.store.constants.view(1, 1, H, W, Cc).expand(idx.numel(), 1, H, W, Cc).contiguous()
    return inp, tgt, forc, const


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(H, W, B, S, T, iters, rounds, packing=None):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feed_latency.py needs the GPU")
    ds = build(H, W, T, S)
    dev = ds.store.device
    n_t = ds.n_time_inputs
    # device tables of the composed path, uploaded once like the kernel's plane table
    ds._in_cols_dev, ds._out_cols_dev = (torch.tensor(c, device=dev) for c in (ds.in_columns, ds.out_columns))
    ds._kind_in_dev = torch.as_tensor(np.tile(ds.kind_in, n_t), device=dev)
    ds._p0_in_dev, ds._p1_in_dev = (torch.as_tensor(np.tile(v, n_t), device=dev) for v in (ds.p0_in, ds.p1_in))
    ds._kind_out_dev, ds._p0_out_dev, ds._p1_out_dev = (torch.as_tensor(v, device=dev)
                                                        for v in (ds.kind_out, ds.p0_out, ds.p1_out))
    g = torch.Generator().manual_seed(5)
    sets = [torch.randint(0, len(ds), (B,), generator=g).to(dev) for _ in range(N_INDEX_SETS)]
    shapes = ds.batch_shapes(B)
    out = tuple(torch.empty(s, device=dev) for s in shapes)
    n_values = out[0].numel() + out[1].numel()
    src, dst = torch.randn(n_values, device=dev), torch.empty(n_values, device=dev)
    turn = {"n": 0}

    def next_idx():
        turn["n"] += 1
        return sets[turn["n"] % N_INDEX_SETS]
    fns = {"batch": lambda: ds.batch(next_idx(), out=out),
           "assemble": lambda: ds.assemble(next_idx(), out[0], out[1]),
           "composed": lambda: composed(ds, next_idx()),
           "copy": lambda: dst.copy_(src)}
    if packing:
        from paradis_model_amd import dataset as D
        pds = packed_twin(ds, packing)
        ps = pds.store
        F = ps.shape[1]
        n = min(T, max(1, D.SLAB_BYTES // (F * H * W * 4)))                # the rows of one upload slab
        slab, stage = ds.store.data[:n], torch.empty(n, F, H, W, device=dev)
        codes, params = torch.empty_like(ps.codes[:n]), torch.empty_like(ps.plane_params[:n])
        ws = {}
        fns.update({"assemble_packed": lambda: pds.assemble(next_idx(), out[0], out[1]),
                    "batch_packed": lambda: pds.batch(next_idx(), out=out),
                    "pack": lambda: D.pack_planes(slab, 0, codes, params, ps.domain_dev, ws),
                    "unpack": lambda: D.unpack_planes(ps.codes, ps.plane_params, ps.domain_dev, 0, n, out=stage),
                    "slab_copy": lambda: stage.copy_(slab)})
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                ms[name].append(event_ms(fn, iters))
        got = [t.clone() for t in ds.batch(sets[0], out=out)]
        ref = composed(ds, sets[0])
    same = all(torch.equal(a, b) for a, b in zip(got, ref))
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = 8.0 * n_values
    extra = {}
    if packing:
        slab_values = slab.numel()
        extra = {"packing": packing, "packed_store_GB": round(ps.nbytes / 1e9, 3),
                 "assemble_packed_ms": round(med["assemble_packed"], 5), "batch_packed_ms": round(med["batch_packed"], 5),
                 "packed_over_float_assemble": round(med["assemble_packed"] / med["assemble"], 3),
                 "packed_over_float_batch": round(med["batch_packed"] / med["batch"], 3),
                 "assemble_packed_TBps": round(6.0 * n_values / (med["assemble_packed"] * 1e-3) / 1e12, 3),
                 "slab_rows": n, "slab_MB": round(4.0 * slab_values / 1e6, 2), "pack_ms": round(med["pack"], 5),
                 "unpack_ms": round(med["unpack"], 5), "slab_copy_ms": round(med["slab_copy"], 5),
                 "pack_Gvalues_per_s": round(slab_values / (med["pack"] * 1e-3) / 1e9, 2),
                 "unpack_Gvalues_per_s": round(slab_values / (med["unpack"] * 1e-3) / 1e9, 2),
                 "slab_copy_Gvalues_per_s": round(slab_values / (med["slab_copy"] * 1e-3) / 1e9, 2),
                 "pack_over_slab_copy": round(med["pack"] / med["slab_copy"], 3)}
    return {"device": torch.cuda.get_device_name(0), "grid": f"{H}x{W}", "B": B, "S": S, "store_times": T,
            "store_GB": round(ds.store.data.numel() * 4 / 1e9, 3), "iters": iters, "rounds": rounds,
            "batch_ms": round(med["batch"], 5), "assemble_ms": round(med["assemble"], 5),
            "composed_ms": round(med["composed"], 5), "copy_ms": round(med["copy"], 5),
            **{f"{k}_ms_all": [round(v, 5) for v in vals] for k, vals in ms.items()},
            "algorithmic_MB": round(nbytes / 1e6, 2), "assemble_TBps": round(nbytes / (med["assemble"] * 1e-3) / 1e12, 3),
            "copy_TBps": round(nbytes / (med["copy"] * 1e-3) / 1e12, 3),
            "fraction_of_copy_rate": round(med["copy"] / med["assemble"], 3),
            "composed_over_batch": round(med["composed"] / med["batch"], 2),
            "batch_equals_composed": bool(same), "index_errors": ds.index_errors(), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each configuration's child process, seconds")
    ap.add_argument("--packing", default=None, choices=["u16"], help="also measure the packed store of the same data")
    ap.add_argument("--out", default=None, help="default profiles/feed_latency.json, feed_latency_u16.json with --packing")
    ap.add_argument("--one", default="", help="(internal) H,W,B,S,T,iters: measure one configuration, print JSON")
    a = ap.parse_args()
    if a.one:
        H, W, B, S, T, iters = (int(v) for v in a.one.split(","))
        print("RESULT " + json.dumps(measure(H, W, B, S, T, iters, a.rounds, a.packing)), flush=True)
        return
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "feed_latency_u16.json" if a.packing else "feed_latency.json")
    res = {"tool": "feed_latency", "configs": []}
    for cfg in CONFIGS:
        tag = "x".join(str(v) for v in cfg[:4])
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--one", ",".join(str(v) for v in cfg)]
        if a.packing:
            cmd += ["--packing", a.packing]
        try:
            out = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"feed_latency: {tag} ran out of its {a.limit} s; stopping")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"feed_latency: {tag} ended with {out.returncode}; stopping")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["configs"].append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
