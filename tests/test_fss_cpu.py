"""Neighbourhood verification without a device: the numpy restatement tests/fss_oracle.py against itself (brute force ==
fast) and against known answers, the host side of ``neighbourhood.FractionsTable`` (constructor, half-width tables,
``result`` / ``skilful_scale`` / ``table`` from hand-made accumulators) and the C ABI of csrc/fss.hip (symbols, limits,
refusals before any HIP call).  Integers are compared exactly; float64 host formulas against hand-computed values at
rtol 1e-12."""
import ctypes
import os

import numpy as np
import pytest
import torch

from paradis_model_amd import neighbourhood as NB
from tests import events_oracle as EO
from tests import fss_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tp", "u10", "v10", "t2m"]
EV1 = {"rain": {"source": "tp", "thresholds": [0.5]}}


def fill(table, lead, cnt, n_samples):
    """the oracle's int64 arrays of one lead into the accumulator of a (CPU) table, in the entry point's layout"""
    TM, head = table.tmax, table.head
    acc = table.acc[lead]
    for s, n in enumerate(table.n_thresholds):
        acc[s, :, 0] = torch.from_numpy(cnt["valid"][s])
        acc[s, :, 1:1 + n] = torch.from_numpy(cnt["forecast_yes"][s, :, :n])
        acc[s, :, 1 + TM:1 + TM + n] = torch.from_numpy(cnt["observed_yes"][s, :, :n])
        for k in range(len(table.scales)):
            for j in range(n):
                for q, key in enumerate(("ff", "oo", "fo")):
                    acc[s, :, head + 3 * (k * TM + j) + q] = torch.from_numpy(cnt[key][s, :, k, j])
    table.n_samples[lead] = n_samples


# ================================================================================================ 1. the oracle
@pytest.mark.parametrize("case", [
    ("ny larger than H", 2, 2, 4, 7, 6, [1, 0, 2, 1]),
    ("2 nx + 1 == W", 1, 1, 3, 7, 1, [3, 3, 3]),
    ("2 nx + 1 == W - 1", 2, 1, 3, 8, 2, [3, 3, 3]),
    ("row-dependent nx", 2, 3, 6, 9, 2, [4, 0, 1, 2, 3, 0]),
    ("a single row and the cell itself", 3, 2, 1, 5, 0, [0]),
], ids=lambda c: c[0])
def test_oracle_brute_force_equals_fast(case):
    _, B, n, H, W, ny, nx = case
    rng = np.random.default_rng(H * 100 + W)
    F, O = rng.random((B, n, H, W)) < 0.4, rng.random((B, n, H, W)) < 0.3
    brute = FO.window_sums_brute(F, O, ny, np.array(nx))
    fast = FO.window_sums_fast(F, O, ny, np.array(nx))
    for a, b in zip(brute, fast):
        assert a.dtype == b.dtype == np.int64 and a.shape == (H, n) and np.array_equal(a, b)
    assert brute[0].sum() > 0 and brute[2].sum() > 0


def _displaced(H, W, row, wf, wo):
    f, t = np.zeros((1, 1, H, W), np.float32), np.zeros((1, 1, H, W), np.float32)
    f[0, 0, row, wf] = t[0, 0, row, wo] = 1.0
    return f, t


def test_displaced_cell_known_answer():
    """one forecast event cell d = 3 columns from the one truth cell, uniform weights, square windows of half-width n:
    FF = OO = (2n+1)^2 cells see one event, FO = (2n+1) max(0, 2n+1-d), so fss = max(0, 1 - d / (2n+1))"""
    H, W, scales = 21, 16, [0, 1, 2, 3, 4]
    src = [{"kind": "plain", "c0": 0, "thresholds": [0.5], "direction": "ge"}]
    hx = NB.half_x_table(scales, np.linspace(-80, 80, H), W, "cells")
    assert np.array_equal(hx, np.repeat(np.array(scales, np.int32)[:, None], H, 1))
    inner = FO.counts(*_displaced(H, W, 10, 4, 7), src, scales, hx)
    dateline = FO.counts(*_displaced(H, W, 10, W - 2, 1), src, scales, hx)
    for k in FO.KEYS:
        assert np.array_equal(inner[k], dateline[k]), k
    for k, n in enumerate(scales):
        side = 2 * n + 1
        assert inner["ff"][0, :, k, 0].sum() == inner["oo"][0, :, k, 0].sum() == side * side
        assert inner["fo"][0, :, k, 0].sum() == side * max(0, side - 3)
    for cnt in (inner, dateline):
        table = NB.FractionsTable(["tp"], np.linspace(-80, 80, H), W, 1, EV1, scales, weights=np.ones(H), device="cpu")
        fill(table, 0, cnt, 1)
        res = table.result()
        np.testing.assert_allclose(res["fss"][0, 0, 0, :, 0], [0.0, 0.0, 0.4, 4.0 / 7.0, 2.0 / 3.0], rtol=1e-12, atol=0)
        assert res["base_rate"][0, 0, 0, 0] == 1.0 / (H * W) and res["frequency_bias"][0, 0, 0, 0] == 1.0
        assert res["valid_fraction"][0, 0, 0] == 1.0


def test_scale_zero_is_the_contingency_table():
    """ny = nx = 0: cF = F, cO = O, so FF == nF, OO == nO and FO is the joint count of the events oracle"""
    rng = np.random.default_rng(3)
    B, H, W = 2, 5, 9
    f = rng.standard_normal((B, 4, H, W)).astype(np.float32)
    t = rng.standard_normal((B, 4, H, W)).astype(np.float32)
    clim = rng.standard_normal((2, 4, H, W)).astype(np.float32)
    f[0, 0, 2, 3], t[1, 1, 0, 0], clim[1, 3, 4, 8] = np.nan, np.inf, np.nan
    srcs = [{"kind": "plain", "c0": 0, "thresholds": [-0.5, 0.25], "direction": "ge"},
            {"kind": "speed", "c0": 1, "c1": 2, "thresholds": [1.0], "direction": "le"},
            {"kind": "anomaly", "c0": 3, "thresholds": [0.0, 0.5, -0.5], "direction": "ge"}]
    kidx = np.array([1, 0])
    ev = EO.counts(f, t, srcs, clim, kidx)
    got = FO.counts(f, t, srcs, [0], np.zeros((1, H), np.int64), clim, kidx, window_sums=FO.window_sums_brute)
    assert np.array_equal(got["valid"], ev["valid"])
    assert np.array_equal(got["forecast_yes"], ev["forecast_yes"]) and np.array_equal(got["observed_yes"], ev["observed_yes"])
    assert np.array_equal(got["ff"][:, :, 0], ev["forecast_yes"]) and np.array_equal(got["oo"][:, :, 0], ev["observed_yes"])
    assert np.array_equal(got["fo"][:, :, 0], ev["both"])
    assert (ev["valid"] < B * W).any()


# ================================================================================================ 2. the host side
def test_metric_half_widths_on_a_grid_with_poles():
    H, W = 33, 64
    lat = np.linspace(-90.0, 90.0, H)                  # dlat = 5.625 = dlon
    lim = NB.limits()
    cap = min(lim["max_half_x"], (W - 1) // 2)
    assert cap == 31
    hx = NB.half_x_table([0, 1, 4], lat, W, "metric")
    assert hx.dtype == np.int32 and hx.shape == (3, H)
    assert (hx[0] == 0).all()                           # the cell itself at every latitude, the poles too
    assert hx[1, 0] == hx[1, -1] == hx[2, 0] == hx[2, -1] == cap
    assert hx[1, 16] == 1 and hx[2, 16] == 4            # the equator: square in cells
    for k, ny in ((1, 1), (2, 4)):
        for h in range(1, H - 1):
            want = min(cap, int(np.floor(ny / np.cos(np.deg2rad(lat[h])) + 0.5)))
            assert hx[k, h] == want, (k, h)
    assert hx[2, 1] == cap and hx[2, 8] == 6            # 4 / cos(84.375 deg) = 40.8 -> the cap; 4 / cos(45 deg) = 5.66 -> 6
    assert np.array_equal(hx, hx[:, ::-1])
    table = NB.FractionsTable(NAMES, lat, W, 1, EV1, [0, 1, 4], "metric", device="cpu")
    assert np.array_equal(table.half_x, hx)
    rows = np.array([[1] * H, [2] + [3] * (H - 2) + [2], [5, 6, 7, 8] + [9] * (H - 8) + [8, 7, 6, 5]])
    assert np.array_equal(table.window_cells, rows * (2 * hx.astype(np.int64) + 1))
    cells = NB.FractionsTable(NAMES, lat, 8, 1, EV1, [0, 2, 16], device="cpu")
    assert cells.half_x[:, 0].tolist() == [0, 2, 3]      # "cells": nx = ny, capped at (W - 1) // 2
    with pytest.raises(ValueError, match="two latitudes"):
        NB.half_x_table([1], np.zeros(1), W, "metric")


def test_constructor_refusals():
    H, W = 5, 8
    lat = np.linspace(-60, 60, H)
    lim = NB.limits()
    good = dict(names=NAMES, lat_deg=lat, n_lon=W, n_leads=2, events=EV1, scales=[0, 1], device="cpu")

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            NB.FractionsTable(**{**good, **kw})

    NB.FractionsTable(**good)
    refused("FractionsTable: names", names=[])
    refused("n_leads", n_leads=0)
    refused("n_leads", n_leads=True)
    refused("n_lon", n_lon=0)
    refused("n_lon", n_lon=2.5)
    refused("lat_deg", lat_deg=[0.0, 91.0])
    refused("weights", weights=np.ones(H + 1))
    refused("weights", weights=-np.ones(H))
    refused("FractionsTable: bands", bands={})
    refused("FractionsTable:", bands={"x": (50.0, 40.0)})
    refused("climatology", climatology=torch.zeros(1, 4, H, W + 1))
    refused("climatology", climatology=torch.zeros(1, 4, H, W, dtype=torch.float64))
    refused("FractionsTable: events must be", events={})
    refused("FractionsTable: event 'rain': channel", events={"rain": {"source": "nope", "thresholds": [1.0]}})
    refused("FractionsTable: event 'w' is an anomaly", events={"w": {"source": ("anomaly", "t2m"), "thresholds": [0.0]}})
    refused("FractionsTable: event 'rain' has 9 thresholds", events={"rain": {"source": "tp", "thresholds": list(range(9))}})
    refused("scales, 1 to", scales=[])
    refused("scales, 1 to", scales=[0] * (lim["max_scales"] + 1))
    refused("scales must be", scales=3)
    refused("a scale must be", scales=[0, -1])
    refused("a scale must be", scales=[0, lim["max_half_y"] + 1])
    refused("a scale must be", scales=[0, 1.5])
    refused("lon_scaling", lon_scaling="km")
    refused("half_x must be an integer table", half_x=np.zeros((2, H + 1), np.int32))
    refused("half_x must be an integer table", half_x=np.zeros((2, H)))
    refused(r"half_x must lie in \[0, 3\]", half_x=np.full((2, H), 4))
    refused(r"half_x must lie in", half_x=-np.ones((2, H), np.int64))
    wide = NB.FractionsTable(**{**good, "n_lon": 1440, "half_x": np.full((2, H), lim["max_half_x"])})
    assert wide.half_x.dtype == np.int32 and wide.acc.shape == (2, 1, H, 1 + 2 * 8 + 3 * lim["max_scales"] * 8)
    refused(r"half_x must lie in \[0, 64\]", n_lon=1440, half_x=np.full((2, H), lim["max_half_x"] + 1))


def test_update_argument_errors_on_cpu_tensors():
    H, W = 5, 8
    lat = np.linspace(-60, 60, H)
    table = NB.FractionsTable(NAMES, lat, W, 2, EV1, [0, 1], device="cpu")
    x = torch.zeros(2, 4, H, W)
    for match, args in (("lead", (2, x, x)), ("lead", (True, x, x)), (r"\[B, C, H, W\]", (0, x[0], x)),
                        ("float32", (0, x.double(), x)), ("longitudes", (0, torch.zeros(2, 4, H, W + 1), x)),
                        ("truth is", (0, x, x[:1])), ("dense", (0, torch.zeros(2, 4, H, 2 * W)[..., ::2], x)),
                        ("no climatology", (0, x, x, torch.zeros(2, dtype=torch.int32)))):
        with pytest.raises(ValueError, match=match):
            table.update(*args)
    with pytest.raises(RuntimeError, match="MI355X"):
        table.update(0, x, x)
    with_clim = NB.FractionsTable(NAMES, lat, W, 2, EV1, [0], climatology=torch.zeros(2, 4, H, W), device="cpu")
    with pytest.raises(ValueError, match="clim_index is needed"):
        with_clim.update(0, x, x)
    with pytest.raises(ValueError, match="int32 tensor"):
        with_clim.update(0, x, x, torch.zeros(2))


def test_result_skilful_scale_and_table_from_hand_made_counts():
    """two rows, uniform weights 1 and 3, scales ny = 0, 1 with nx = 0, 1 (N = 1 and, clipped to two rows, 2 * 3 = 6),
    two leads (the second never updated), a source with two thresholds beside one with one"""
    H, W = 2, 4
    ev = {"a": {"source": "tp", "thresholds": [1.0, 2.0]}, "b": {"source": "t2m", "thresholds": [0.0], "direction": "le"}}
    table = NB.FractionsTable(NAMES, [-10.0, 10.0], W, 2, ev, [0, 1], weights=np.array([1.0, 3.0]),
                              bands={"all": (-90, 90), "north": (0, 90)}, device="cpu")
    assert np.array_equal(table.window_cells, [[1, 1], [6, 6]])
    cnt = {"valid": np.array([[8, 8], [8, 6]]),
           "forecast_yes": np.array([[[2, 0], [4, 0]], [[1, -1], [0, -1]]]),
           "observed_yes": np.array([[[4, 0], [2, 0]], [[2, -1], [0, -1]]]),
           #           row 0: k=0 (j0, j1), k=1 (j0, j1)        row 1
           "ff": np.array([[[[2, 0], [60, 0]], [[4, 0], [72, 0]]], [[[1, -1], [9, -1]], [[0, -1], [9, -1]]]]),
           "oo": np.array([[[[4, 0], [90, 0]], [[2, 0], [36, 0]]], [[[2, -1], [36, -1]], [[0, -1], [18, -1]]]]),
           "fo": np.array([[[[1, 0], [66, 0]], [[1, 0], [45, 0]]], [[[0, -1], [18, -1]], [[0, -1], [9, -1]]]])}
    fill(table, 0, cnt, 2)
    got = table.counts()
    for k in FO.KEYS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k][0], cnt[k]), k
        assert (np.where(cnt[k] < 0, -1, 0) == got[k][1]).all(), k
    assert got["n_samples"].tolist() == [2, 0]
    res = table.result()
    assert res["fss"].shape == res["fbs"].shape == res["fbs_ref"].shape == (2, 2, 2, 2, 2)
    assert res["base_rate"].shape == res["frequency_bias"].shape == res["fss_uniform"].shape == (2, 2, 2, 2)
    # source a, threshold 0, band "all": rows weighted 1 and 3
    num0 = 1.0 * (2 + 4 - 2) + 3.0 * (4 + 2 - 2)
    ref0 = 1.0 * (2 + 4) + 3.0 * (4 + 2)
    num1 = (1.0 * (60 + 90 - 132) + 3.0 * (72 + 36 - 90)) / 36.0
    ref1 = (1.0 * (60 + 90) + 3.0 * (72 + 36)) / 36.0
    np.testing.assert_allclose(res["fbs"][0, 0, 0, :, 0], [num0, num1], rtol=1e-12)
    np.testing.assert_allclose(res["fbs_ref"][0, 0, 0, :, 0], [ref0, ref1], rtol=1e-12)
    np.testing.assert_allclose(res["fss"][0, 0, 0, :, 0], [1 - num0 / ref0, 1 - num1 / ref1], rtol=1e-12)
    base = (1.0 * 4 + 3.0 * 2) / (1.0 * 8 + 3.0 * 8)
    np.testing.assert_allclose(res["base_rate"][0, 0, 0, 0], base, rtol=1e-12)
    np.testing.assert_allclose(res["frequency_bias"][0, 0, 0, 0], (2 + 12) / (4 + 6), rtol=1e-12)
    np.testing.assert_allclose(res["fss_uniform"][0, 0, 0, 0], 0.5 + base / 2, rtol=1e-12)
    # band "north": row 1 alone
    np.testing.assert_allclose(res["fss"][0, 0, 1, :, 0], [1 - 4.0 / 6.0, 1 - 18.0 / 108.0], rtol=1e-12)
    # source a, threshold 1: no event anywhere -> fbs_ref == 0 -> NaN, the sums themselves are 0
    assert np.isnan(res["fss"][0, 0, :, :, 1]).all() and (res["fbs_ref"][0, 0, :, :, 1] == 0).all()
    assert np.isnan(res["frequency_bias"][0, 0, :, 1]).all() and (res["base_rate"][0, 0, :, 1] == 0).all()
    # source b has one threshold: NaN past it; lead 1 was never updated: NaN everywhere
    for k in ("fss", "fbs", "fbs_ref"):
        assert np.isnan(res[k][0, 1, :, :, 1]).all() and np.isnan(res[k][1]).all(), k
    for k in ("base_rate", "frequency_bias", "fss_uniform"):
        assert np.isnan(res[k][0, 1, :, 1]).all() and np.isnan(res[k][1]).all(), k
    # source b, "north": no event in row 1 itself (NaN at the cell scale), but its 2 x 3 windows reach into row 0
    assert np.isnan(res["fss"][0, 1, 1, 0, 0]) and res["fbs_ref"][0, 1, 1, 0, 0] == 0.0
    np.testing.assert_allclose(res["fss"][0, 1, 1, 1, 0], 1 - (9 + 18 - 18) / (9 + 18), rtol=1e-12)
    # source b, "all": cell scale 1 - 3 / 3 = 0; windows 1 - (9 + 3 * 9) / (45 + 3 * 27)
    np.testing.assert_allclose(res["fss"][0, 1, 0, :, 0], [0.0, 1 - 36.0 / 126.0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["valid_fraction"][0], [[1.0, 1.0], [(8 + 18) / 32.0, 0.75]], rtol=1e-12)
    assert np.isnan(res["valid_fraction"][1]).all()
    assert res["count"].tolist() == [2, 0] and res["labels"] == ["a", "b"] and res["scales"] == [0, 1]
    assert res["thresholds"] == [[1.0, 2.0], [0.0]] and res["directions"] == ["ge", "le"]
    assert res["bands"] == ["all", "north"] and np.array_equal(res["window_cells"], table.window_cells)
    # skilful scale: a / all: fss = 0.333.., 0.8286 against uniform 0.65625 -> scale 1; a / north: 0.333, 0.8333 against
    # 0.5 + 0.125 -> 1; threshold 1 and the dead entries: -1
    first = table.skilful_scale(res)
    assert first.shape == (2, 2, 2, 2) and first.dtype == np.int64
    assert first[0, 0, :, 0].tolist() == [1, 1] and (first[0, 0, :, 1] == -1).all() and (first[1] == -1).all()
    assert first[0, 1, 0, 0] == 1               # b / all: 0 and 0.714 against 0.5 + (2 / 26) / 2
    res["fss"][0, 0, 0, 0, 0] = 0.9
    assert NB.skilful_scale(res)[0, 0, 0, 0] == 0
    res["fss"][0, 0, 0, :, 0] = 0.65            # below 0.65625 at every scale
    assert NB.skilful_scale(res)[0, 0, 0, 0] == -1
    text = table.table(res, "a", "north")
    lines = text.splitlines()
    assert lines[0] == "a / north" and "fss >=1" in lines[1] and "ny=0" in lines[1] and "ny=1" in lines[1]
    assert "0.3333" in lines[2] and "0.8333" in lines[2] and lines[2].split()[1] == "2" and lines[2].split()[-1] == "1"
    assert "fss <=0" in table.table(res, "b")
    with pytest.raises(ValueError, match="labels"):
        table.table(res, "c")
    with pytest.raises(ValueError, match="bands"):
        table.table(res, "a", "south")
    table.reset()
    assert int(table.acc.abs().sum()) == 0 and int(table.n_samples.sum()) == 0


def test_forecaster_run_refusals_with_fractions():
    from paradis_model_amd.forecast import Forecaster, PostSpec
    H, W = 5, 8
    lat = np.linspace(-60, 60, H)
    names = NAMES[:3]
    spec = PostSpec.from_features(names, [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    fc = Forecaster(None, spec, lat, np.zeros(W), graph=False)
    inp, forc, const = torch.zeros(1, 1, 6, H, W), torch.zeros(1, 2, H, W, 1), torch.zeros(1, 1, H, W, 1)
    table = lambda n=2, nm=names: NB.FractionsTable(nm, lat, W, n, EV1, [0, 1], device="cpu")     # noqa: E731
    with pytest.raises(ValueError, match="fractions table needs truth"):
        fc.run(inp, forc, const, None, fractions=table(), truth=None)
    good = torch.zeros(1, 2, 3, H, W)
    args = (None, good, False, None, 1, 2, 3, H, W, None, None)
    with pytest.raises(ValueError, match="truth"):
        fc._check_verification(None, good[:, :1], False, None, 1, 2, 3, H, W, None, None, table())
    with pytest.raises(ValueError, match="fractions table has 1 leads"):
        fc._check_verification(*args, table(1))
    with pytest.raises(ValueError, match="fractions table's names"):
        fc._check_verification(*args, table(2, ["tp", "v10", "u10"]))
    with pytest.raises(ValueError, match="clim_index must be int32"):
        fc._check_verification(None, good, False, torch.zeros(1, 2), 1, 2, 3, H, W, None, None, table())
    with pytest.raises(RuntimeError, match="MI355X"):                   # every host check passed: the device check
        fc._check_verification(*args, table())


# ================================================================================================ 3. the C ABI
SYMBOLS = ("paradis_fss_max_scales", "paradis_fss_max_half_y", "paradis_fss_max_half_x", "paradis_fss_max_w",
           "paradis_fss_rows", "paradis_fss_ws_bytes", "paradis_fss_update")


def test_fss_symbols_limits_and_abi():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    sig = _lib.SIGNATURES["paradis_fss_update"][1]
    assert len(sig) == 21 and sig[1] is ctypes.c_int64 and sig[3] is ctypes.c_int64 and sig[6] is ctypes.c_int
    assert _lib.SIGNATURES["paradis_fss_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert _lib.SIGNATURES["paradis_fss_rows"] == (ctypes.c_int, [ctypes.c_int] * 2)
    L = _lib.lib
    assert L.paradis_abi_version() == 10
    assert L.paradis_fss_max_scales() >= 4 and L.paradis_fss_max_half_y() >= 16
    assert L.paradis_fss_max_half_x() >= 64 and L.paradis_fss_max_w() >= 1440
    for W in (1, 64, 1440):
        for ny in (0, 1, L.paradis_fss_max_half_y()):
            assert L.paradis_fss_rows(W, ny) >= 1
    assert L.paradis_fss_rows(0, 1) == 0 and L.paradis_fss_rows(64, -1) == 0
    assert L.paradis_fss_rows(L.paradis_fss_max_w() + 1, 1) == 0 and L.paradis_fss_rows(64, L.paradis_fss_max_half_y() + 1) == 0
    with open(os.path.join(ROOT, "paradis_model_amd", "csrc", "Makefile")) as f:
        assert "FLAGS_fss := -ffp-contract=off" in f.read()


def test_fss_workspace_holds_the_bits_and_the_partials():
    """uint16 [B][S][H][W] rounded up to 16 bytes, then uint64 [B][S][H][1 + 2 TMAX + 3 K TMAX]; 0 for empty shapes"""
    from paradis_model_amd import _lib
    L = _lib.lib
    for (B, S, H, W, K) in ((2, 3, 32, 64, 3), (1, 3, 721, 1440, 5), (3, 1, 1, 5, 1), (1, 1, 3, 5, L.paradis_fss_max_scales())):
        bits = (B * S * H * W * 2 + 15) // 16 * 16
        assert L.paradis_fss_ws_bytes(B, S, H, W, K) == bits + B * S * H * (17 + 24 * K) * 8
    for shape in ((0, 3, 32, 64, 2), (2, 0, 32, 64, 2), (2, 3, 0, 64, 2), (2, 3, 32, 0, 2), (2, 3, 32, 64, 0),
                  (2, 3, 32, 64, L.paradis_fss_max_scales() + 1)):
        assert L.paradis_fss_ws_bytes(*shape) == 0


def test_fss_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first
    TM = L.paradis_events_max_thresholds()
    tables = {}

    def call(word, fc=fake, truth=fake, clim=None, idx=None, Kc=0, src=((0, 0, 0, 1),), sign=1.0, hy=(0, 1), hx=fake,
             acc=fake, n=fake, ws=fake, B=2, C=3, S=None, H=4, W=8, K=None, fc_bs=96, truth_bs=96, no_table=None):
        st = np.ascontiguousarray(np.array(src, np.int32).reshape(-1, 4))
        tt = np.zeros((len(st), 1 + TM), np.float32)
        tt[:, 0] = sign
        yy = np.ascontiguousarray(np.array(hy, np.int32))
        tables.update(src=st.ctypes.data, thr=tt.ctypes.data, hy=yy.ctypes.data)
        if no_table:
            tables[no_table] = None
        S = len(st) if S is None else S
        K = len(yy) if K is None else K
        rc = L.paradis_fss_update(fc, fc_bs, truth, truth_bs, clim, idx, Kc, tables["src"], tables["thr"], tables["hy"], hx,
                                  acc, n, ws, B, C, S, H, W, K, None)
        assert rc == 1 and word in _lib.last_error(), (word, rc, _lib.last_error())

    call("bad shape", B=-1)
    call("bad shape", C=0)
    call("bad shape", H=0)
    call("bad shape", W=0)
    call("bad shape", S=0)
    call("bad shape", src=((0, 0, 0, 1),) * (L.paradis_events_max_sources() + 1))
    call("longitudes", W=L.paradis_fss_max_w() + 1, fc_bs=1 << 40, truth_bs=1 << 40)
    call("scales", K=0)
    call("scales", hy=(0,) * (L.paradis_fss_max_scales() + 1))
    call("half_y", hy=(0, -1))
    call("half_y", hy=(L.paradis_fss_max_half_y() + 1,))
    call("null table", no_table="src")
    call("null table", no_table="thr")
    call("null table", no_table="hy")
    call("go together", clim=fake)
    call("go together", idx=fake)
    call("K_clim must be", clim=fake, idx=fake, Kc=0)
    call("grid limit", B=1 << 30, H=721, W=1440, fc_bs=1 << 40, truth_bs=1 << 40)
    call("strides", fc_bs=95)
    call("strides", truth_bs=95)
    call("no climatology", src=((2, 0, 0, 1),))
    call("kind", src=((3, 0, 0, 1),))
    call("channels", src=((0, 3, 0, 1),))
    call("channels", src=((0, -1, 0, 1),))
    call("channels", src=((0, 0, 0, 1), (1, 0, 3, 1)))
    call("thresholds", src=((0, 0, 0, 0),))
    call("thresholds", src=((0, 0, 0, TM + 1),))
    call("sign", sign=0.5)
    call("missing", acc=None)
    call("missing", n=None)
    call("workspace", ws=None)
    call("workspace", ws=ctypes.c_void_p(264))
    call("null input", fc=None)
    call("null input", hx=None)
    # B == 0 does nothing and asks for nothing
    assert L.paradis_fss_update(None, 0, None, 0, None, None, 0, None, None, None, None, None, None, None, 0, 3, 1, 4, 8,
                                1, None) == 0
