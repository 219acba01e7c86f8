"""CPU restatement of the reference's dataset item (``data/era5_dataset.py:337-423``: ``_getitem_standard``,
``_getitem_prediction``, and ``_apply_normalization`` ``:547-584``) over a ``[T, F, H, W]`` tensor, plus the builder of
the small stores the dataset tests run on.

TEST INFRASTRUCTURE ONLY.  Built as the reference builds: channels-last slices, concatenation of the input times along
the last axis, in-place normalisation - by ``oracle.feed_oracle.normalize_features``, which ``f4_feed.pt`` pins to the
reference's own functions - then the permutation to channels-first; forcings by ``feed_oracle.compute_forcings``.  The
feature bookkeeping (``:150-166,266-279``) and the normalisation tables (``:458-544``) are restated here independently
of ``paradis_model_amd.dataset``.
"""
import re
from types import SimpleNamespace

import numpy as np
import torch

from oracle import feed_oracle as FO
from paradis_model_amd.config import default_config, reduced_config

EPS = 1e-12     # era5_dataset.py:58


def feature_lists(cfg):
    """(dyn_input_features, dyn_output_features, n_common): era5_dataset.py:266-276"""
    levels = cfg.features.pressure_levels
    inputs = [f"{v}_h{l}" for v in cfg.features.input.atmospheric for l in levels] + list(cfg.features.input.surface)
    outputs = [f"{v}_h{l}" for v in cfg.features.output.atmospheric for l in levels] + list(cfg.features.output.surface)
    common = [f for f in outputs if f in inputs]
    return (common + [f for f in inputs if f not in outputs], common + [f for f in outputs if f not in inputs],
            len(common))


def norm_tables(names, stats_of, custom, q_min, q_max):
    """kind / p0 / p1 per feature of ``names`` (era5_dataset.py:468-489,516-523): float32 tensors"""
    kind, p0, p1 = [], [], []
    for f in names:
        base = re.sub(r"_h\d+$", "", f)
        if custom and base == "total_precipitation_6hr":
            kind.append(FO.KIND_PRECIP), p0.append(0.0), p1.append(0.0)
        elif custom and base == "specific_humidity":
            kind.append(FO.KIND_HUMIDITY), p0.append(float(q_min)), p1.append(float(q_max))
        else:
            kind.append(FO.KIND_ZSCORE), p0.append(float(stats_of["mean"][f])), p1.append(float(stats_of["std"][f]))
    return kind, torch.tensor(p0, dtype=torch.float32), torch.tensor(p1, dtype=torch.float32)


def humidity_range(in_names, stats_of):
    """(q_min, q_max) of era5_dataset.py:528-540 (float32)"""
    hum = [f for f in in_names if re.sub(r"_h\d+$", "", f) == "specific_humidity"]
    if not hum:
        return torch.tensor(EPS), torch.tensor(0.0)
    q_max = torch.tensor([stats_of["max"][f] for f in hum], dtype=torch.float32).max()
    q_min = torch.tensor([stats_of["min"][f] for f in hum], dtype=torch.float32).min()
    if q_min < EPS:
        q_min = torch.tensor(EPS)
    return q_min, q_max


def item(case, ind, *, n_time_inputs=None, interval_steps=None, prediction_shift=None, steps=None, prediction=False):
    """One dataset item exactly as ``_getitem_standard`` (or ``_getitem_prediction``) assembles it: (x [1, n_t*Fin, H, W],
    y [S, Fout, H, W] or None, forcings [S, H, W, Nf]).  The keyword overrides replace the case's own bookkeeping (the
    self-checks sweep them)."""
    n_t = case.n_time_inputs if n_time_inputs is None else n_time_inputs
    interval = case.interval_steps if interval_steps is None else interval_steps
    shift = case.prediction_shift if prediction_shift is None else prediction_shift
    steps = case.steps if steps is None else steps
    ds = case.store[case.base:]                                          # ds.sel(time=slice(adjusted_start, None)) :137
    times = case.times[case.base:]
    ds_input = ds[:, case.in_cols].permute(0, 2, 3, 1)                   # [time, lat, lon, features] :299
    ds_output = ds[:, case.out_cols].permute(0, 2, 3, 1)
    ind = ind * interval                                                 # :338
    input_ini = ind
    x = ds_input[input_ini:input_ini + n_t].clone()                      # :344-346
    forcing_times = times[input_ini:input_ini + steps + n_t - 1]         # :348-349
    if n_t > 1:
        x = torch.cat([x[j] for j in range(n_t)], dim=-1).unsqueeze(0)   # :365-366
    # n_t == 1: the one-time slice already is [1, lat, lon, features] (the reference's unsqueeze at :368 would make five
    # axes, on which its own permute at :379 fails: the shipped configuration has n_t = 2; this is the item it means)
    kind_in, p0_in, p1_in = case.norm_in
    x = FO.normalize_features(x, kind_in * n_t, p0_in.repeat(n_t), p1_in.repeat(n_t), EPS)   # :551-577
    y = None
    if not prediction:
        output_ini = input_ini + n_t + shift                             # :351
        output_end = ind + steps + n_t + shift                           # :352
        y = ds_output[output_ini:output_end].clone()
        assert y.shape[0] == steps, "the store is too short for this item"
        y = FO.normalize_features(y, *case.norm_out, EPS).permute(0, 3, 1, 2).contiguous()   # :560-584, :380
    forcings = FO.compute_forcings(forcing_times, case.lat.numpy(), case.lon.numpy(), n_t, case.toa_mean, case.toa_std,
                                   case.forcing_inputs)                  # :376
    return x.permute(0, 3, 1, 2).contiguous(), y, forcings               # :379


def batch(case, indices, prediction=False):
    """default collation of ``item`` over ``indices``: (input [B,1,C,H,W], target [B,S,Fout,H,W] | None, forcings,
    constants [B,1,H,W,Cc])"""
    items = [item(case, int(i), prediction=prediction) for i in indices]
    x = torch.stack([it[0] for it in items])
    y = None if prediction else torch.stack([it[1] for it in items])
    f = torch.stack([it[2] for it in items])
    c = case.constants.unsqueeze(0).unsqueeze(0).expand(len(items), 1, -1, -1, -1).contiguous()   # constant_data[:1]
    return x, y, f, c


def small_config(n_time_inputs=2, interval_steps=1, delta_steps=1, standard=False, full=False):
    """``reduced_config`` with two pressure levels, an input-only feature (wind_z_10m is dropped from the outputs; the
    vertical velocity and the precipitation are output-only already) and the dataset keys of the shipped YAML.
    ``full``: the unmodified feature list (what the model tests use)."""
    cfg = reduced_config()
    if not full:
        cfg.features.pressure_levels = [500, 850]
        cfg.features.output.surface = [f for f in cfg.features.output.surface if f != "wind_z_10m"]
    cfg.dataset.n_time_inputs = n_time_inputs
    cfg.dataset.time_resolution = "6h"
    cfg.dataset.sampling_interval = f"{6 * interval_steps}h"
    cfg.dataset.prediction_delta = f"{6 * delta_steps}h"
    cfg.normalization = type(cfg.dataset)({"standard": bool(standard)})
    return cfg


def build_case(H, W, *, n_time_inputs=2, interval_steps=1, delta_steps=1, steps=1, n_samples=4, base=1, seed=0,
               identity=False, full=False, q_min_floor=False):
    """A store, its stats and a matching config.

    The store's feature axis is a seeded shuffle of the configured features plus two that no configuration uses; the first
    sample's first input time sits at store row ``base``; the store ends exactly where the last sample's targets end.
    identity: ``store[t, f, y, x] = t*F + f + (y*W + x)/4096`` (exact in float32), mean 0 / std 1 and
    ``normalization.standard`` - every output plane then names its (t, f).  Otherwise: realistic magnitudes, humidity in
    [0, 1.1 q_max] (so the clip acts) and non-negative precipitation.  q_min_floor: a humidity minimum of 0, which the
    dataset must raise to 1e-12."""
    cfg = small_config(n_time_inputs, interval_steps, delta_steps, standard=identity, full=full)
    n_t = n_time_inputs
    shift = (delta_steps - 1) * interval_steps                           # era5_dataset.py:111-113
    in_names, out_names, n_common = feature_lists(cfg)
    g = torch.Generator().manual_seed(1000 + seed)
    names = sorted(set(in_names + out_names)) + ["unused_field", "unused_level_h500"]
    names = [names[i] for i in torch.randperm(len(names), generator=g).tolist()]
    F = len(names)
    T = base + (n_samples - 1) * interval_steps + n_t + shift + steps
    times = np.datetime64("2000-02-27T00", "us") + np.arange(T) * np.timedelta64(6, "h")
    if identity:
        t_i = torch.arange(T, dtype=torch.float32).view(T, 1, 1, 1)
        f_i = torch.arange(F, dtype=torch.float32).view(1, F, 1, 1)
        cell = (torch.arange(H * W, dtype=torch.float32) / 4096).view(1, 1, H, W)
        store = t_i * F + f_i + cell
        assert T * F < 2 ** 10 and H * W < 2 ** 13                       # 10 + 13 bits < 24: exact
        stats = {"mean": np.zeros(F, np.float32), "std": np.ones(F, np.float32),
                 "min": np.zeros(F, np.float32), "max": np.full(F, float(T * F + 2), np.float32)}
    else:
        mean = (torch.randn(F, generator=g) * 50).numpy().astype(np.float32)
        std = (torch.rand(F, generator=g) * 9 + 0.5).numpy().astype(np.float32)
        store = torch.randn(T, F, H, W, generator=g) * torch.from_numpy(std).view(1, F, 1, 1) \
            + torch.from_numpy(mean).view(1, F, 1, 1)
        mn, mx = mean - 4 * std, mean + 4 * std
        for j, name in enumerate(names):
            bare = re.sub(r"_h\d+$", "", name)
            if bare == "specific_humidity":
                mx[j] = 0.02 / (1 + j % 3)
                mn[j] = 0.0 if q_min_floor else 1e-8 * (1 + j % 2)
                store[:, j] = torch.rand(T, H, W, generator=g) * (1.1 * 0.02)      # above every q_max at times
            elif bare == "total_precipitation_6hr":
                mn[j], mx[j] = 0.0, 0.2
                store[:, j] = torch.rand(T, H, W, generator=g).pow(4) * 0.05
        stats = {"mean": mean, "std": std, "min": mn.astype(np.float32), "max": mx.astype(np.float32)}
    d = 180.0 / H
    lat = (-90.0 + d / 2 + d * torch.arange(H, dtype=torch.float64)).to(torch.float32)
    lon = (torch.arange(W, dtype=torch.float64) * (360.0 / W)).to(torch.float32)
    constants = torch.randn(H, W, len(cfg.features.input.constants), generator=g)
    column = {n: j for j, n in enumerate(names)}
    stats_of = {k: {n: v[column[n]] for n in names} for k, v in stats.items()}
    custom = not identity
    q_min, q_max = humidity_range(in_names, stats_of)
    first = base + n_t - 1                                               # store row of start_date
    last = first + (n_samples - 1) * interval_steps
    return SimpleNamespace(
        cfg=cfg, store=store.contiguous(), times=times, features=names, stats=stats, lat=lat, lon=lon,
        constants=constants, toa_mean=251.3, toa_std=302.7, forcing_inputs=list(cfg.features.input.forcings),
        start_date=str(times[first].astype("datetime64[s]")), end_date=str(times[last].astype("datetime64[s]")),
        n_time_inputs=n_t, interval_steps=interval_steps, prediction_shift=shift, steps=steps, n_samples=n_samples,
        base=base, in_names=in_names, out_names=out_names, n_common=n_common,
        in_cols=[column[n] for n in in_names], out_cols=[column[n] for n in out_names],
        q_min=q_min, q_max=q_max, custom=custom,
        norm_in=norm_tables(in_names, stats_of, custom, q_min, q_max),
        norm_out=norm_tables(out_names, stats_of, custom, q_min, q_max))


def make_store(case, device):
    """the ``DeviceStore`` of a case"""
    from paradis_model_amd.dataset import DeviceStore
    return DeviceStore(case.store.numpy(), case.times, case.features, case.stats, case.lat, case.lon, case.constants,
                       case.toa_mean, case.toa_std, device=device)


def make_dataset(case, device, prediction_stage=False):
    from paradis_model_amd.dataset import DeviceDataset
    return DeviceDataset(make_store(case, device), case.cfg, case.start_date, case.end_date, case.steps,
                         prediction_stage=prediction_stage)
