"""Plain fp64 numpy restatements for the store preparation (paradis_model_amd/prepare.py, csrc/prepare.hip): the
reference's Cartesian-wind formula and two-pass per-feature statistics, plus the seeded inputs the golden generator
(tests/golden/make_golden_prepare.py) and the tests share.  The wind formula is checked against the reference's own
output (tests/golden/p1_prepare.pt) by tests/test_prepare_cpu.py."""
import numpy as np

G, R = 9.80616, 287.05
LEVELS = [300, 850, 1000]                       # hPa
WIND_T = 2                                      # time rows of the wind cases
WIND_GRIDS = [(9, 16, True), (8, 15, False)]    # (H, W, poles)


def grid_deg(nlat, nlon, poles):
    """float64 degrees: latitudes ascending with or without the poles, longitudes from 0"""
    if poles:
        lat = np.linspace(-90.0, 90.0, nlat)
    else:
        d = 180.0 / nlat
        lat = -90.0 + d / 2 + d * np.arange(nlat)
    return lat, np.arange(nlon) * (360.0 / nlon)


def wind_fields(seed, T, L, H, W):
    """float32 u, v [T, L, H, W] (m/s), omega (Pa/s), temperature (K), u10, v10 [T, H, W]"""
    g = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)        # noqa: E731
    return {"u": f32(g.normal(0, 15, (T, L, H, W))), "v": f32(g.normal(0, 10, (T, L, H, W))),
            "w": f32(g.normal(0, 0.4, (T, L, H, W))), "t": f32(g.normal(260, 25, (T, L, H, W))),
            "u10": f32(g.normal(0, 6, (T, H, W))), "v10": f32(g.normal(0, 5, (T, H, W)))}


def cartesian_wind(lat_deg, lon_deg, levels, f):
    """The reference's compute_cartesian_wind for float32 fields and float64 grids, every type written out: numpy keeps
    omega * R * T in float32 (a float32 array times a Python scalar times a float32 array) and evaluates the rest in
    float64, left to right.  Returns float64 (x, y, z [T, L, H, W], x10, y10, z10 [T, H, W]) and, for the error bound of
    the tests, the sums of the magnitudes of the terms of each (same shapes)."""
    lat, lon = np.deg2rad(np.asarray(lat_deg, np.float64))[:, None], np.deg2rad(np.asarray(lon_deg, np.float64))[None, :]
    sla, cla, slo, clo = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    u, v = f["u"].astype(np.float64), f["v"].astype(np.float64)
    wrt = (f["w"] * np.float32(R)) * f["t"]
    assert wrt.dtype == np.float32
    k = wrt.astype(np.float64) / (np.asarray(levels, np.float64)[:, None, None] * 100 * G)
    tx = (-u * slo, v * sla * clo, k * cla * clo)
    ty = (u * clo, v * sla * slo, k * cla * slo)
    tz = (v * cla, k * sla)
    u10, v10 = f["u10"].astype(np.float64), f["v10"].astype(np.float64)
    sx = (-u10 * slo, v10 * sla * clo)
    sy = (u10 * clo, v10 * sla * slo)
    sz = (v10 * cla,)
    val = (tx[0] - tx[1] - tx[2], ty[0] - ty[1] - ty[2], tz[0] - tz[1], sx[0] - sx[1], sy[0] - sy[1], sz[0])
    mag = tuple(sum(np.abs(t) for t in terms) for terms in (tx, ty, tz, sx, sy, sz))
    return val, mag


def wind_names(levels):
    """(source names, destination names) of a store that holds the raw fields and the Cartesian winds side by side, a
    feature the plan does not name at either end"""
    src = ["geopotential_h500"]
    for l in levels:
        src += [f"u_component_of_wind_h{l}", f"v_component_of_wind_h{l}", f"vertical_velocity_h{l}", f"temperature_h{l}"]
    src += ["10m_u_component_of_wind", "10m_v_component_of_wind"]
    dst = [f"wind_{a}_h{l}" for l in levels for a in "xyz"] + ["wind_x_10m", "wind_y_10m", "wind_z_10m", "2m_temperature"]
    return src, dst


def pack_sources(names, levels, f):
    """[T, len(names), H, W] float32: the fields at their named columns, every other column a ramp"""
    T, _, H, W = f["u"].shape
    out = np.empty((T, len(names), H, W), np.float32)
    out[:] = np.arange(out.size, dtype=np.float32).reshape(out.shape) * np.float32(0.25)
    col = {n: j for j, n in enumerate(names)}
    for i, l in enumerate(levels):
        for key, var in (("u", "u_component_of_wind"), ("v", "v_component_of_wind"), ("w", "vertical_velocity"),
                         ("t", "temperature")):
            out[:, col[f"{var}_h{l}"]] = f[key][:, i]
    out[:, col["10m_u_component_of_wind"]] = f["u10"]
    out[:, col["10m_v_component_of_wind"]] = f["v10"]
    return out


def stats_store(seed, T, H, W):
    """[T, 6, H, W] float32: N(2e5, 3e3); |N| 1e-6; N(1e5, 0.5) (sum x^2 cancels); the constant 7.25; N(0, 1) with one
    NaN cell and one all-NaN row; NaN everywhere"""
    g = np.random.default_rng(seed)
    x = np.empty((T, 6, H, W), np.float64)
    x[:, 0] = g.normal(2e5, 3e3, (T, H, W))
    x[:, 1] = np.abs(g.normal(0, 1, (T, H, W))) * 1e-6
    x[:, 2] = g.normal(1e5, 0.5, (T, H, W))
    x[:, 3] = 7.25
    x[:, 4] = g.normal(0, 1, (T, H, W))
    x[1, 4, H // 2, W // 3] = np.nan
    x[T - 2, 4, H - 1, :] = np.nan
    x[:, 5] = np.nan
    return x.astype(np.float32)


def _five(x):
    """two-pass fp64 statistics over every axis but 1; float32 results, int64 count"""
    import warnings
    x = x.astype(np.float64)
    ax = (0, 2, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN features
        m = np.nanmean(x, axis=ax)
        s = np.sqrt(np.nanmean((x - m[None, :, None, None]) ** 2, axis=ax))
        lo, hi = np.nanmin(x, axis=ax), np.nanmax(x, axis=ax)
    f32 = lambda a: a.astype(np.float32)                         # noqa: E731
    return {"mean": f32(m), "std": f32(s), "min": f32(lo), "max": f32(hi), "count": np.isfinite(x).sum(axis=ax) +
            np.isinf(x).sum(axis=ax)}


def statistics(x, strides=()):
    """mean / std (ddof 0) / min / max / count per feature of x [T, F, H, W] float32, NaN skipped, and per stride the same
    of the float32 difference x[s:] - x[:-s] with n_samples = T - s"""
    out = _five(x)
    out["tendencies"] = {}
    for s in strides:
        d = x[s:] - x[:-s]
        assert d.dtype == np.float32
        t = _five(d)
        out["tendencies"][s] = {"tendency_mean": t["mean"], "tendency_std": t["std"], "tendency_min": t["min"],
                                "tendency_max": t["max"], "count": t["count"], "n_samples": x.shape[0] - s}
    return out


def ulps32(a, b):
    """distance in float32 ulps, elementwise; 0 where both are NaN, a large number where one is"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    both, one = np.isnan(a) & np.isnan(b), np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(one, 1 << 40, d))
