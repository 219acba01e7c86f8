"""CPU restatement of the forecast writer's layout and encoding (paradis_model_amd/encode.py, csrc/encode.hip), written
from the reference's ``utils/file_output.py`` and numcodecs' published ``BitRound.encode`` for the tests: BitRound on
float32 bit patterns, the regrouping of a chunk into named variables (``_build_dataset_for_samples``), the region
bookkeeping (``write_forecast_region_chunked``), the store template (``_build_template_dataset``), the initial state
(``init_data``) and the seeded raw store the golden generator and the GPU tests share.

TEST INFRASTRUCTURE ONLY, independent of ``paradis_model_amd.encode``.  ``utils/file_output.py`` needs xarray / dask to
import and numcodecs is not installed: its loops and the BitRound arithmetic are restated here, not called.  The wind
conversion and the dew point of the initial state ARE pinned to the reference's own functions by
tests/golden/e1_encode.pt (tests/test_encode_cpu.py)."""
import re

import numpy as np
import torch

from tests import forecast_oracle as FO

ATM_RENAMES = (("wind_x", "u_component_of_wind"), ("wind_y", "v_component_of_wind"), ("wind_z", "vertical_velocity"))
SFC_RENAMES = (("wind_x_10m", "10m_u_component_of_wind"), ("wind_y_10m", "10m_v_component_of_wind"))


# ---------------------------------------------------------------------------------- BitRound
def bitround(x, keepbits):
    """float32 array -> float32 array of the rounded bit patterns (a copy).  ``keepbits`` 1 .. 23, or None: unchanged.
    uint32 arithmetic wraps as the int32 arithmetic of the published code does; the kept bit and the mask are the same
    bits either way."""
    a = np.ascontiguousarray(x, dtype=np.float32).copy()
    if keepbits is None or keepbits == 23:
        return a
    assert 1 <= keepbits < 23
    b = a.view(np.uint32)
    maskbits = 23 - keepbits
    half_quantum1 = np.uint32((1 << (maskbits - 1)) - 1)
    with np.errstate(over="ignore"):
        b += ((b >> np.uint32(maskbits)) & np.uint32(1)) + half_quantum1
    b &= np.uint32((0xFFFFFFFF << maskbits) & 0xFFFFFFFF)
    return a


def bits(x):
    """the int32 view the tests compare on"""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------- variables
def replace_variable_names(cfg):
    atm, sfc = list(cfg.features.output.atmospheric), list(cfg.features.output.surface)
    for old, new in ATM_RENAMES:
        atm = [new if v == old else v for v in atm]
    for old, new in SFC_RENAMES:
        sfc = [new if v == old else v for v in sfc]
    return atm, sfc


def variable_indices(cfg, names, levels):
    """name -> ("atm", [channel per level]) | ("sfc", channel), in the order and with the overwrites of the reference's
    ``data_vars`` dict"""
    atm, sfc = replace_variable_names(cfg)
    idx = {f: i for i, f in enumerate(names)}
    out = {}
    for src, dst in zip(cfg.features.output.atmospheric, atm):
        out[dst] = ("atm", [idx[f"{src}_h{level}"] for level in levels])
    for src, dst in zip(cfg.features.output.surface, sfc):
        if src == "wind_z_10m":
            continue
        out[dst] = ("sfc", idx[src])
    return out


def variables(cfg, names, levels, forecast, dew, init=None, init_dew=None, keepbits=16, dewpoint=True):
    """The encoded ``data_vars`` of one chunk: forecast [B, n, C, H, W] and dew [B, n, L, H, W] float32 numpy, the
    initial state ``init`` [B, 1, C, H, W] / ``init_dew`` [B, 1, L, H, W] prepended when given; every value BitRounded."""
    fc = np.asarray(forecast, np.float32)
    dw = None if dew is None else np.asarray(dew, np.float32)
    if init is not None:
        fc = np.concatenate((np.asarray(init, np.float32), fc), axis=1)
        if dewpoint:
            dw = np.concatenate((np.asarray(init_dew, np.float32), dw), axis=1)
    out = {}
    for name, (kind, ind) in variable_indices(cfg, names, levels).items():
        out[name] = bitround(fc[:, :, ind], keepbits)
    if dewpoint:
        out["dewpoint_depression"] = bitround(dw, keepbits)
    return out


# ---------------------------------------------------------------------------------- regions and template
def sorted_time_info(times):
    """``_get_sorted_time_info``: (sorted times, map dataset index -> sorted position)"""
    raw = np.asarray(times)
    order = np.argsort(raw)
    pos = np.empty_like(order)
    pos[order] = np.arange(len(order))
    return raw[order], pos


def regions(sample_indices, sample_index_to_sorted_pos, start_idx, n):
    """[(batch rows in ascending sample order, (time start, stop), (timedelta start, stop))] per run of consecutive
    sorted positions"""
    s = np.asarray(sample_indices)
    order = np.argsort(s)
    positions = np.asarray(sample_index_to_sorted_pos)[s[order]]
    breaks = np.where(np.diff(positions) != 1)[0] + 1
    td = (1 + start_idx, 1 + start_idx + n) if start_idx > 0 else (0, 1 + n)
    return [(order[g].tolist(), (int(positions[g[0]]), int(positions[g[-1]]) + 1), td)
            for g in np.split(np.arange(len(positions)), breaks)]


def template(cfg, names, levels, n_time, forecast_steps, output_frequency, H, W):
    """name -> (dims, shape, chunks) of the float variables of ``_build_template_dataset``, and total_pred_steps"""
    total = (forecast_steps - 1) // output_frequency + 1 + 1
    L = len(levels)
    atm, sfc = replace_variable_names(cfg)
    out = {}
    for v in atm:
        out[v] = (5, (n_time, total, L, H, W), (1, min(10, total), L, H, W))
    for v in sfc:
        if v == "wind_z_10m":
            continue
        out[v] = (4, (n_time, total, H, W), (1, min(10, total), H, W))
    out["dewpoint_depression"] = (5, (n_time, total, L, H, W), (1, min(10, total), L, H, W))
    return out, total


# ---------------------------------------------------------------------------------- the initial state
def feature_lists(cfg):
    """(single-time input features, output features) as data/era5_dataset.py:266-276 orders them"""
    levels = cfg.features.pressure_levels
    inputs = [f"{v}_h{l}" for v in cfg.features.input.atmospheric for l in levels] + list(cfg.features.input.surface)
    outputs = [f"{v}_h{l}" for v in cfg.features.output.atmospheric for l in levels] + list(cfg.features.output.surface)
    common = [f for f in outputs if f in inputs]
    return common + [f for f in inputs if f not in outputs], common + [f for f in outputs if f not in inputs]


def store_features(cfg, seed):
    """the feature axis of the seeded store: a seeded shuffle of every configured feature plus one nobody uses"""
    ins, outs = feature_lists(cfg)
    names = sorted(set(ins + outs)) + ["unused_field"]
    g = torch.Generator().manual_seed(seed)
    return [names[i] for i in torch.randperm(len(names), generator=g).tolist()]


def raw_store(seed, features, T, H, W):
    """seeded raw (physical-unit) store [T, F, H, W] float32: temperatures 250 +- 15 K, specific humidity in
    (1e-6, 0.02), precipitation >= 0, everything else N(mean, std) with seeded mean / std"""
    g = torch.Generator().manual_seed(seed)
    F = len(features)
    mean = torch.randn(F, generator=g) * 10
    std = torch.rand(F, generator=g) * 5 + 0.5
    x = torch.randn(T, F, H, W, generator=g) * std.view(1, F, 1, 1) + mean.view(1, F, 1, 1)
    u = torch.rand(T, F, H, W, generator=g)
    for j, f in enumerate(features):
        b = re.sub(r"_h\d+$", "", f)
        if b in ("temperature", "2m_temperature"):
            x[:, j] = 250.0 + 15.0 * (2 * u[:, j] - 1)
        elif b == "specific_humidity":
            x[:, j] = 1e-6 + 0.02 * u[:, j]
        elif b == "total_precipitation_6hr":
            x[:, j] = 0.05 * u[:, j].pow(4)
    return x.contiguous()


def init_rows(base, n_time_inputs, interval_steps, indices):
    """store rows of the samples' init times"""
    return [base + n_time_inputs - 1 + int(i) * interval_steps for i in indices]


def gathered_init(store, features, rows, input_features, output_features):
    """``init_data`` of ``_build_dataset_for_samples`` before the wind conversion: [B, 1, C, H, W], NaN where an output
    is not an input"""
    store = np.asarray(store)
    col = {f: j for j, f in enumerate(features)}
    input_data = store[rows][:, [col[f] for f in input_features]]               # [B, F_in, H, W]
    init = np.full((len(rows), 1, len(output_features)) + store.shape[2:], np.nan, dtype=store.dtype)
    where = {f: i for i, f in enumerate(input_features)}
    for o, f in enumerate(output_features):
        if f in where:
            init[:, 0, o] = input_data[:, where[f]]
    return init


def initial_state(store, features, rows, input_features, output_features, levels, lat_deg, lon_deg):
    """(init_data after the wind conversion [B, 1, C, H, W], dew-point depression of it [B, 1, L, H, W]), float32"""
    init = gathered_init(store, features, rows, input_features, output_features)
    q = init[:, :, FO.indices("specific_humidity", output_features)].copy()
    T = init[:, :, FO.indices("temperature", output_features)].copy()
    FO.spherical_winds(init, output_features, levels, lat_deg, lon_deg)
    return init, FO.dewpoint_depression(q, T, levels)
