"""Plain numpy fp64 restatement of the verification climatology (paradis_model_amd/climatology.py), for the tests:
slots and weights from ``datetime64`` arithmetic written independently of ``ClimPlan`` (a loop over rows and window
offsets), the NaN-skipping weighted mean in float64, winds from ``tests/forecast_oracle.spherical_winds``.  Test
infrastructure; reads nothing outside the repository."""
import math

import numpy as np

from tests import forecast_oracle as FO


def case_times():
    """2019-12-01 .. 2021-02-01 at 12 h spacing: covers 29 Feb 2020 and two New Years (857 rows)"""
    return np.arange(np.datetime64("2019-12-01T00", "h"), np.datetime64("2021-02-01T00", "h") + 1,
                     np.timedelta64(12, "h")).astype("datetime64[us]")


def day_of_year(day):
    """1..366 of a datetime64[D] scalar"""
    return int((day - day.astype("datetime64[Y]").astype("datetime64[D]")) / np.timedelta64(1, "D")) + 1


def weight(delta, weights, sigma_days):
    return 1.0 if weights == "boxcar" else math.exp(-(delta * delta) / (2.0 * sigma_days * sigma_days))


def slot_lists(times, *, start=None, end=None, hours=None, days=None, window_days=1, weights="boxcar",
               sigma_days=None):
    """per slot the list of (row, weight), rows ascending; (lists, hours, days).  ``start`` / ``end``: datetime64
    bounds, both inclusive."""
    times = np.asarray(times).astype("datetime64[us]")
    keep = [i for i, t in enumerate(times) if (start is None or t >= start) and (end is None or t <= end)]
    hour_of = [int((t - t.astype("datetime64[D]")) / np.timedelta64(1, "h")) for t in times]
    if hours is None:
        hours = sorted({hour_of[i] for i in keep})
    hours = sorted(hours)
    days = list(range(1, 367)) if days is None else list(days)
    half = window_days // 2
    lists = [[] for _ in range(len(days) * len(hours))]
    for i in keep:                                        # ascending rows: every slot's list comes out ascending
        if hour_of[i] not in hours:
            continue
        day = times[i].astype("datetime64[D]")
        for delta in range(-half, half + 1):
            d = day_of_year(day + np.timedelta64(delta, "D"))
            if d in days:
                lists[days.index(d) * len(hours) + hours.index(hour_of[i])].append((i, weight(delta, weights, sigma_days)))
    return lists, hours, days


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    rows = np.array([r for l in lists for r, _ in l], np.int64)
    w = np.array([x for l in lists for _, x in l], np.float64)
    return ptr, rows, w


def slot_means(x, lists, cols):
    """x [T, F, H, W] float32 numpy -> float64 [K, C, H, W]: sum w x / sum w over the finite values per pixel, in list
    order; NaN where no entry is finite"""
    T, F, H, W = x.shape
    out = np.full((len(lists), len(cols), H, W), np.nan)
    for k, entries in enumerate(lists):
        if not entries:
            continue
        S = np.zeros((len(cols), H, W))
        Wt = np.zeros((len(cols), H, W))
        for row, w in entries:
            v = x[row][cols].astype(np.float64)
            ok = np.isfinite(v)
            S += np.where(ok, w * np.where(ok, v, 0.0), 0.0)
            Wt += np.where(ok, w, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[k] = np.where(Wt > 0, S / Wt, np.nan)
    return out


def climatology(x, lists, cols, names=None, levels=None, lat_deg=None, lon_deg=None):
    """(float64 means [K, C, H, W], the means rounded to float32 once, and - with ``names`` - a copy whose wind triples
    were turned by ``forecast_oracle.spherical_winds``: float64 from the rounded means, one more rounding; else None)"""
    mean = slot_means(x, lists, cols)
    plain = mean.astype(np.float32)
    turned = None
    if names is not None:
        turned = plain.copy()
        with np.errstate(invalid="ignore"):
            FO.spherical_winds(turned, list(names), levels, lat_deg, lon_deg)
    return mean, plain, turned
