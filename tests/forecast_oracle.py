"""CPU restatement of the forecast post-processing (row f5), written from the formulas, for the tests: feature
classes, de-normalisation, Cartesian -> spherical winds in float64, dew-point depression, the chunk bookkeeping of the
predict loop, and the seeded inputs / statistics the golden generator uses.  Checked against the reference's own
outputs (tests/golden/f5_post.pt, f5_forecast.pt) by tests/test_forecast_cpu.py."""
import re

import numpy as np
import torch

G, R = 9.80616, 287.05
EPS1, EPS2 = 0.6219800221014, 0.3780199778986


def base_name(f):
    return re.sub(r"_h\d+$", "", f)


def indices(name, names):
    return [i for i, f in enumerate(names) if base_name(f) == name]


def classes(names, custom):
    """(precipitation, humidity, z-score) channel lists"""
    pr = [i for i, f in enumerate(names) if custom and base_name(f) == "total_precipitation_6hr"]
    hu = [i for i, f in enumerate(names) if custom and base_name(f) == "specific_humidity"]
    zs = [i for i in range(len(names)) if i not in pr and i not in hu]
    return pr, hu, zs


def channel_stats(names, seed=501):
    """per-channel (mean, std) float32 for all channels: temperatures 250 / 15 K (keeps T > 180 K), humidity and
    precipitation at their physical scale (used when they are z-scored), everything else seeded"""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(len(names), generator=g) * 10
    std = torch.rand(len(names), generator=g) * 5 + 0.5
    for i, f in enumerate(names):
        b = base_name(f)
        if b in ("temperature", "2m_temperature"):
            mean[i], std[i] = 250.0, 15.0
        elif b == "specific_humidity":
            mean[i], std[i] = 5e-3, 2e-3
        elif b == "total_precipitation_6hr":
            mean[i], std[i] = 1e-3, 1e-3
    return mean, std


Q_MIN, Q_MAX = 1e-7, 0.025


def normalised_state(seed, names, *shape):
    """seeded normalised state [..., C, H, W] with C = len(names) at dim -3: N(0,1), humidity channels U(-0.1, 1.1),
    precipitation U(-4.5, 7)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    u = torch.rand(*shape, generator=g)
    for i, f in enumerate(names):
        b = base_name(f)
        if b == "specific_humidity":
            x[..., i, :, :] = u[..., i, :, :] * 1.2 - 0.1
        elif b == "total_precipitation_6hr":
            x[..., i, :, :] = u[..., i, :, :] * 11.5 - 4.5
    return x


def denormalise(x, names, mean_all, std_all, custom, q_min=Q_MIN, q_max=Q_MAX, eps=1e-12):
    """x [..., C, H, W] float32 -> physical units, float32 torch arithmetic"""
    pr, hu, zs = classes(names, custom)
    y = x.clone()
    if pr:
        y[..., pr, :, :] = torch.clip(torch.exp(x[..., pr, :, :] - 10) - 1e-6, min=0)
    if hu:
        lmin, lmax = torch.log(torch.tensor(q_min)), torch.log(torch.tensor(q_max))
        y[..., hu, :, :] = torch.clip(torch.exp(x[..., hu, :, :] * (lmax - lmin) + lmin) - eps, min=0, max=q_max)
    y[..., zs, :, :] = x[..., zs, :, :] * std_all[zs].view(-1, 1, 1) + mean_all[zs].view(-1, 1, 1)
    return y


def spherical_winds(y, names, levels, lat_deg, lon_deg):
    """in place on a float32 numpy array [..., C, H, W]; float64 evaluation from float64 degrees, one rounding"""
    lat = np.deg2rad(np.asarray(lat_deg, np.float64))[:, None]
    lon = np.deg2rad(np.asarray(lon_deg, np.float64))[None, :]
    sla, cla, slo, clo = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    it, ix, iy, iz = (indices(v, names) for v in ("temperature", "wind_x", "wind_y", "wind_z"))
    p = np.asarray([float(v) for v in levels])[:, None, None]
    T = y[..., it, :, :].copy()
    X, Y, Z = (y[..., i, :, :].astype(np.float64) for i in (ix, iy, iz))
    y[..., ix, :, :] = -X * slo + Y * clo
    y[..., iy, :, :] = -X * sla * clo - Y * sla * slo + Z * cla
    y[..., iz, :, :] = (-X * cla * clo - Y * cla * slo - Z * sla) * (p * 100 * G / (np.float32(R) * T))
    sx, sy, sz = (indices(v, names) for v in ("wind_x_10m", "wind_y_10m", "wind_z_10m"))
    if sx:
        X, Y, Z = (y[..., i, :, :].astype(np.float64) for i in (sx, sy, sz))
        y[..., sx, :, :] = -X * slo + Y * clo
        y[..., sy, :, :] = -X * sla * clo - Y * sla * slo + Z * cla
    return y


def dewpoint_depression(q, T, levels):
    """q, T float32 numpy [..., L, H, W]; pressure = integer hPa * 100; float64 evaluation, float32 result"""
    p = (np.asarray(levels).astype(np.int64) * 100).astype(np.float64)[:, None, None]
    hu = np.maximum(np.float32(1e-10), q.astype(np.float32))
    den = np.float32(EPS1) + np.float32(EPS2) * hu                   # float32, as numpy keeps it
    e = np.minimum(p, hu.astype(np.float64) * p / den.astype(np.float64))
    c = np.log(e / 610.94)
    td = (30.11 * c - 17.625 * 273.16) / (c - 17.625)
    return np.minimum(T.astype(np.float64) - td, 30.0).astype(np.float32)


def postprocess(x, names, levels, mean_all, std_all, custom, lat_deg, lon_deg):
    """normalised torch [..., C, H, W] -> (physical float32 numpy, dew-point depression float32 numpy)"""
    y = denormalise(x, names, mean_all, std_all, custom).numpy()
    q = y[..., indices("specific_humidity", names), :, :].copy()
    T = y[..., indices("temperature", names), :, :].copy()
    spherical_winds(y, names, levels, lat_deg, lon_deg)
    return y, dewpoint_depression(q, T, levels)


def plan_events(S, freq, n=None):
    """the predict loop's bookkeeping as a list of events: ("store", step, slot, start_idx of its chunk) and
    ("flush", after step, start_idx, states)"""
    n = S if n is None else n
    ev, buf, start, stored = [], 0, None, 0
    for step in range(S):
        if step % freq == 0:
            if start is None:
                start = stored
            ev.append(("store", step, buf, start))
            buf += 1
            stored += 1
            if buf == n:
                ev.append(("flush", step, start, buf))
                buf, start = 0, None
    if buf:
        ev.append(("flush", S - 1, start, buf))
    return ev


def events_of_plan(plan):
    """paradis_model_amd.forecast.chunk_plan output -> the same event list"""
    ev, start, stored = [], None, 0
    for step, p in enumerate(plan):
        if p.stored:
            if p.slot == 0:
                start = stored
            ev.append(("store", step, p.slot, start))
            stored += 1
        if p.flush is not None:
            ev.append(("flush", step, p.flush[0], p.flush[1]))
    return ev


def grid_deg(nlat, nlon, poles, dtype=np.float64):
    if poles:
        lat = np.linspace(-90.0, 90.0, nlat)
    else:
        d = 180.0 / nlat
        lat = -90.0 + d / 2 + d * np.arange(nlat)
    return lat.astype(dtype), (np.arange(nlon) * (360.0 / nlon)).astype(dtype)
