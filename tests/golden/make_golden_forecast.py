#!/usr/bin/env python3
"""Generates tests/golden/f5_post.pt and tests/golden/f5_forecast.pt (+ f5_forecast_tail.pt) by importing the
REFERENCE's own post-processing (utils/postprocessing.py, utils/normalization.py, utils/mhuaes.py under
/root/reference) and driving the reference model through a restated ``predict_step`` loop (trainer.py:731-815;
Lightning is not importable, as for c2_rollout).  Run in the build container only.  Only data is stored: recipes and
checksums of the seeded inputs (tests/forecast_oracle.py regenerates them), the reference's outputs, index lists.

  f5_post.pt       8x16 and 9x16, B = 2, one state, 97 channels: _denormalize_dataset + convert_cartesian_to_spherical_winds
                   for custom_normalization true / false and float32 / float64 lat / lon; get_var_indices lists; mhuaes3
  f5_forecast.pt   the chunk bookkeeping for six (S, output_frequency, write_every_n); the rollout (variant "a", 16x32,
                   B = 2, S = 5, output_frequency 2, write_every_n 2): first chunk
  f5_forecast_tail.pt   the rollout's trailing partial chunk (kept apart: no committed file above 1 MiB)
The model state of the rollout is g4_model_a.pt["state"] (same construction; asserted here)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG                                         # noqa: E402  (puts /root/reference on sys.path)
from utils import postprocessing as PP                           # noqa: E402
from utils.mhuaes import mhuaes3                                 # noqa: E402
from tests import forecast_oracle as FO                          # noqa: E402


def names_levels():
    cfg = MG.load_cfg()
    levels = list(cfg.features.pressure_levels)
    in_atm = [f"{v}_h{l}" for v in cfg.features.input.atmospheric for l in levels]
    out_atm = [f"{v}_h{l}" for v in cfg.features.output.atmospheric for l in levels]
    in_f = in_atm + list(cfg.features.input.surface)
    out_f = out_atm + list(cfg.features.output.surface)
    common = [f for f in out_f if f in in_f]
    return cfg, common + [f for f in out_f if f not in in_f], levels


def dataset_stub(names, custom, mean_all, std_all):
    """the attributes _denormalize_dataset reads, built as data/era5_dataset.py:463-523 builds them"""
    pr, hu, zs = [], [], []
    import re
    for i, f in enumerate(names):
        b = re.sub(r"_h\d+$", "", f)
        if b == "total_precipitation_6hr" and custom:
            pr.append(i)
        elif b == "specific_humidity" and custom:
            hu.append(i)
        else:
            zs.append(i)
    zs_t = torch.tensor(zs, dtype=torch.long)
    return types.SimpleNamespace(
        custom_normalization=custom, norm_precip_out=torch.tensor(pr, dtype=torch.long),
        norm_humidity_out=torch.tensor(hu, dtype=torch.long), norm_zscore_out=zs_t,
        output_mean=mean_all[zs_t], output_std=std_all[zs_t],
        q_min=torch.tensor(FO.Q_MIN), q_max=torch.tensor(FO.Q_MAX))


def reference_post(x, names, cfg, ds, lat, lon):
    """what predict_step does to a stacked chunk [B, T, C, H, W] (trainer.py:772-778)"""
    t = x.clone()
    PP.denormalize_datasets(None, t, ds)
    a = t.numpy()
    PP.convert_cartesian_to_spherical_winds(lat, lon, cfg, a, list(names))
    return a


def f5_post():
    cfg, names, levels = names_levels()
    mean_all, std_all = FO.channel_stats(names)
    out = {"numpy": np.__version__, "names": names, "levels": levels, "stats_seed": 501, "cases": {},
           "indices": {v: PP.get_var_indices(v, names).tolist() for v in (
               "temperature", "specific_humidity", "wind_x", "wind_y", "wind_z", "wind_x_10m", "wind_y_10m",
               "wind_z_10m")}}
    for (H, W, poles, seed) in ((8, 16, False, 601), (9, 16, True, 602)):
        x = FO.normalised_state(seed, names, 2, 1, len(names), H, W)
        rec = {"H": H, "W": W, "poles": poles, "seed": seed, "chk": MG.chk(x)}
        for custom in (True, False):
            ds = dataset_stub(names, custom, mean_all, std_all)
            rec[f"zscore_{custom}"] = ds.norm_zscore_out.tolist()
            for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
                lat, lon = FO.grid_deg(H, W, poles, dt)
                rec[f"custom{int(custom)}_{tag}"] = torch.from_numpy(reference_post(x, names, cfg, ds, lat, lon)[:, 0].copy())
            # the writer's derived variable on the float32 de-normalised q and T (wind conversion does not touch them)
            y = rec[f"custom{int(custom)}_f64"].numpy()
            q = y[:, out["indices"]["specific_humidity"]]
            T = y[:, out["indices"]["temperature"]]
            ps = (np.asarray(levels) * 100)[:, None, None]                   # integer hPa * 100, as the writer builds it
            assert ps.dtype.kind == "i" and q.dtype == np.float32
            rec[f"dew_custom{int(custom)}"] = torch.from_numpy(mhuaes3(q, T, ps).astype("float32"))
        assert float(rec["custom1_f64"][:, out["indices"]["temperature"]].min()) > 180.0
        out["cases"][f"{H}x{W}"] = rec
    path = os.path.join(HERE, "f5_post.pt")
    torch.save(out, path)
    print("wrote f5_post.pt", os.path.getsize(path), "bytes")


def restated_predict(model, inp, forc, const, S, freq, n, on_chunk, ncom=83):
    """trainer.py:745-813 line by line, events recorded"""
    events = []
    constants = const[:, :1].permute(0, 1, 4, 2, 3)
    buf, start, stored = [], None, 0
    cur = inp
    for step in range(S):
        if model is not None:
            fs = forc[:, step].unsqueeze(1).permute(0, 1, 4, 2, 3)
            mi = torch.cat([cur, fs, constants], dim=2).squeeze(1)
            with torch.no_grad():
                y = model(mi)
            cur = torch.cat([mi[:, ncom:2 * ncom], y[:, :ncom]], dim=1).unsqueeze(1)
        else:
            y = None
        if step % freq == 0:
            if start is None:
                start = stored
            events.append(("store", step, len(buf), start))
            buf.append(y)
            stored += 1
            if len(buf) == n:
                events.append(("flush", step, start, len(buf)))
                on_chunk(buf, start)
                buf, start = [], None
    if buf:
        events.append(("flush", S - 1, start, len(buf)))
        on_chunk(buf, start)
    return events


def f5_forecast():
    plans = {}
    for (S, freq, n) in ((1, 1, None), (5, 1, 2), (5, 2, 2), (6, 2, None), (7, 3, 1), (4, 1, 8)):
        plans[(S, freq, n)] = restated_predict(None, None, None, torch.zeros(1, 1, 1, 1, 1), S, freq,
                                               S if n is None else n, lambda b, s: None)
    cfg, model, lat_deg, lg, og = MG.build_model("a")
    torch.manual_seed(4242)
    with torch.no_grad():
        for nm, p in model.named_parameters():          # as g4_models
            if nm.endswith((".A", ".U", ".V")):
                p.normal_(0, 0.2)
            elif nm.endswith("ChannelNorm.bias") or (nm.endswith(".bias") and p.dim() == 1):
                p.normal_(0, 0.1)
            elif nm == "alpha_adv":
                p.normal_(-1.0, 0.5)
    g4 = torch.load(os.path.join(HERE, "g4_model_a.pt"), weights_only=False)["state"]
    for k, v in model.state_dict().items():
        assert torch.equal(v, g4[k]), k
    model.eval()
    _, names, levels = names_levels()
    mean_all, std_all = FO.channel_stats(names)
    ds = dataset_stub(names, True, mean_all, std_all)
    H, W = lg.shape
    B, S, freq, n = 2, 5, 2, 2
    inp = MG.seeded(177, B, 1, 166, H, W)
    forc = MG.seeded(179, B, S, H, W, 10, kind="rand")
    const = MG.seeded(180, B, 1, H, W, 10)
    lat, lon = FO.grid_deg(H, W, False, np.float64)
    chunks = []

    def on_chunk(buf, start):
        chunks.append((start, torch.from_numpy(reference_post(torch.stack(buf, dim=1), names, cfg, ds, lat, lon).copy())))

    ev = restated_predict(model, inp, forc, const, S, freq, n, on_chunk)
    assert ev == FO.plan_events(S, freq, n) and [c[1].shape[1] for c in chunks] == [2, 1]
    rec = {"plans": plans, "rollout": {
        "variant": "a", "state_from": "g4_model_a.pt", "seeds": [177, 179, 180], "B": B, "S": S,
        "output_frequency": freq, "write_every_n": n, "chk": MG.chk(inp) + MG.chk(forc) + MG.chk(const),
        "stats_seed": 501, "names": names, "levels": levels, "events": ev, "n_chunks": len(chunks),
        "start_idx": [c[0] for c in chunks], "chunk0": chunks[0][1]}}
    for name, obj in (("f5_forecast.pt", rec), ("f5_forecast_tail.pt", {"chunk1": chunks[1][1]})):
        path = os.path.join(HERE, name)
        torch.save(obj, path)
        print("wrote", name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["post", "forecast"]
    if "post" in which:
        f5_post()
    if "forecast" in which:
        f5_forecast()
