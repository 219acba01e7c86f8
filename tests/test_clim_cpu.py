"""CPU: the host plan of the verification climatology (paradis_model_amd/climatology.py ``ClimPlan``) against the
independent datetime64 loop of tests/clim_oracle.py, its parameters and refusals, and the C interface of the new entry
points (header, signature table and library agree).

Times: 2019-12-01 .. 2021-02-01 at 12 h spacing - 29 Feb 2020 and two New Years."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import clim_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("paradis_clim_mean_chunk", "paradis_clim_mean", "paradis_clim_mean_packed",
               "paradis_spherical_winds_inplace")
WINDOWS = (1, 5, 61)
WEIGHTS = (("boxcar", None), ("gaussian", 2.5))


def _climatology():
    from paradis_model_amd import climatology
    return climatology


@functools.lru_cache(maxsize=None)
def _times():
    t = CO.case_times()
    t.setflags(write=False)
    return t


def _us(t):
    return np.asarray(t).astype("datetime64[us]").astype(np.int64)


def _plan(**kw):
    return _climatology().ClimPlan(_us(_times()), **kw)


@functools.lru_cache(maxsize=None)
def _oracle(window, weights="boxcar", sigma=None):
    lists, hours, days = CO.slot_lists(_times(), window_days=window, weights=weights, sigma_days=sigma)
    return lists, hours, days


@pytest.mark.parametrize("weights,sigma", WEIGHTS)
@pytest.mark.parametrize("window", WINDOWS)
def test_lists_equal_the_oracle(window, weights, sigma):
    lists, hours, days = _oracle(window, weights, sigma)
    kw = {} if sigma is None else {"sigma_days": sigma}
    plan = _plan(window_days=window, weights=weights, **kw)
    assert plan.hours == hours == [0, 12] and plan.days == days and plan.n_slots == 366 * 2
    ptr, rows, w = plan.lists()
    optr, orows, ow = CO.csr(lists)
    assert ptr.dtype == np.int64 and rows.dtype == np.int64 and w.dtype == np.float64
    assert np.array_equal(ptr, optr) and np.array_equal(rows, orows)
    assert np.array_equal(w, ow)                  # exp of the same double argument, or exactly 1
    assert np.array_equal(plan.entries, np.diff(optr))
    for k in range(plan.n_slots):
        assert bool((np.diff(rows[ptr[k]:ptr[k + 1]]) > 0).all()), f"slot {k}: rows not ascending"
    if weights == "gaussian":
        assert w.max() == 1.0 and (window == 1 or w.min() < 1.0)


def test_day_366_and_the_new_year_wrap():
    t = _times()
    dates = t.astype("datetime64[D]")
    plan = _plan(window_days=1)
    ptr, rows, _ = plan.lists()
    for h in (0, 1):
        k = plan.days.index(366) * 2 + h
        got = rows[ptr[k]:ptr[k + 1]]
        assert got.size == 1 and dates[got[0]] == np.datetime64("2020-12-31")      # the only day 366 in the range
    # window 5: day 366 hears 2020-12-29 .. 2021-01-02 and nothing of the turn 2019 / 2020, where no day 366 exists
    plan5 = _plan(window_days=5)
    ptr, rows, _ = plan5.lists()
    k = plan5.days.index(366) * 2
    got = sorted(str(d) for d in dates[rows[ptr[k]:ptr[k + 1]]])
    assert got == ["2020-12-29", "2020-12-30", "2020-12-31", "2021-01-01", "2021-01-02"]
    assert [sorted(r for r, _ in l) for l in _oracle(5)[0]][k] == sorted(rows[ptr[k]:ptr[k + 1]].tolist())
    # ... and a row on 30 Dec contributes to the slot of 1 Jan (delta = +2), in both winters
    k = plan5.days.index(1) * 2
    got = {str(d) for d in dates[rows[ptr[k]:ptr[k + 1]]]}
    assert {"2019-12-30", "2020-12-30"} <= got
    assert "2019-12-29" not in got and "2020-12-29" not in got          # 2020-12-29 + 2 days is day 366
    # 29 Feb: day 60 of the leap year, 1 March is day 61 there and day 60 in 2021 (outside the range)
    k = plan.days.index(60) * 2
    ptr, rows, _ = plan.lists()
    assert [str(d) for d in dates[rows[ptr[k]:ptr[k + 1]]]] == ["2020-02-29"]


def test_start_end_hours_and_days():
    t = _times()
    plan = _plan(start="2020-01-01", end="2020-12-31", window_days=1)
    _, rows, _ = plan.lists()
    assert t[rows.min()] == np.datetime64("2020-01-01T00") and t[rows.max()] == np.datetime64("2020-12-31T12")
    assert plan.entries.sum() == 366 * 2 and bool((plan.entries == 1).all())
    lists, _, _ = CO.slot_lists(t, start=np.datetime64("2020-01-01T00:00:00"), end=np.datetime64("2020-12-31T23:59:59"))
    assert np.array_equal(plan.lists()[1], CO.csr(lists)[1])
    # an explicit clock in start
    assert _plan(start="2020-01-01T12:00:00", end="2020-01-01").entries.sum() == 1

    only0 = _plan(hours=(0,), window_days=1)
    assert only0.hours == [0] and only0.n_slots == 366
    hour = (t - t.astype("datetime64[D]")) / np.timedelta64(1, "h")
    assert bool((hour[only0.lists()[1]] == 0).all()) and only0.entries.sum() == int((hour == 0).sum())

    sub = _plan(days=[1, 60, 366], window_days=5)
    assert sub.n_slots == 3 * 2 and sub.days == [1, 60, 366]
    lists, _, _ = CO.slot_lists(t, days=[1, 60, 366], window_days=5)
    for a, b in zip(sub.lists(), CO.csr(lists)):
        assert np.array_equal(a, b)
    # the order of `days` is the order of the slots
    rev = _plan(days=[366, 1], window_days=1)
    assert rev.slot_of(_us(np.datetime64("2020-12-31T12"))) == 1 and rev.slot_of(_us(np.datetime64("2021-01-01T00"))) == 2


def test_slot_of_round_trips_and_refuses():
    t = _times()
    plan = _plan(window_days=1)
    slots = plan.slot_of(_us(t))
    assert slots.dtype == np.int32 and slots.shape == t.shape
    ptr, rows, _ = plan.lists()
    for k in range(plan.n_slots):                            # a window of one day: a slot's entries are its own times
        assert bool((slots[rows[ptr[k]:ptr[k + 1]]] == k).all())
    two_d = plan.slot_of(torch.from_numpy(_us(t[:6])).reshape(2, 3))
    assert two_d.shape == (2, 3) and np.array_equal(two_d.reshape(-1), slots[:6])
    assert plan.slot_of(_us(np.datetime64("2031-03-01T12"))) == (60 - 1) * 2 + 1       # any year has the slot

    sub = _plan(days=[1, 60, 366], hours=(0,))
    assert sub.slot_of(_us(np.datetime64("2024-02-29T00"))) == 1
    with pytest.raises(ValueError, match="2020-03-05"):
        sub.slot_of(_us(np.array(["2020-02-29T00", "2020-03-05T00", "2020-03-06T00"], "datetime64[h]")))
    with pytest.raises(ValueError, match="2020-02-29T12"):
        sub.slot_of(_us(np.datetime64("2020-02-29T12")))
    with pytest.raises(ValueError, match="2020-02-29T00:30"):
        sub.slot_of(_us(np.datetime64("2020-02-29T00:30")))


def test_refusals():
    C = _climatology()
    us = _us(_times())
    off = us.copy()
    off[7] += 30 * 60 * 1000000
    with pytest.raises(ValueError, match="whole hour"):
        C.ClimPlan(off)
    C.ClimPlan(off, start="2019-12-10")                      # the row is outside start..end: it does not contribute
    for bad in (0, 2, 4, -1, 367, 2.5):
        with pytest.raises(ValueError, match="window_days"):
            C.ClimPlan(us, window_days=bad)
    with pytest.raises(ValueError, match="sigma_days"):
        C.ClimPlan(us, window_days=5, weights="gaussian")
    with pytest.raises(ValueError, match="sigma_days"):
        C.ClimPlan(us, window_days=5, weights="gaussian", sigma_days=0.0)
    with pytest.raises(ValueError, match="weights"):
        C.ClimPlan(us, weights="triangle")
    with pytest.raises(ValueError, match="days"):
        C.ClimPlan(us, days=[0, 1])
    with pytest.raises(ValueError, match="days"):
        C.ClimPlan(us, days=[5, 5])
    with pytest.raises(ValueError, match="hours"):
        C.ClimPlan(us, hours=[24])


def test_build_refuses_on_the_host():
    """the refusals of ``build`` that need no device: a CPU store, other times, a missing name, winds without a spec"""
    from paradis_model_amd.dataset import DeviceStore
    C = _climatology()
    t = _times()[:4]
    feats = ["temperature_h500", "total_precipitation_6hr"]
    st = {k: np.ones(2, np.float32) for k in ("mean", "std", "min", "max")}
    store = DeviceStore(np.zeros((4, 2, 3, 4), np.float32), t, feats, st, np.linspace(-60, 60, 3), np.arange(4) * 90.0,
                        np.zeros((3, 4, 1), np.float32), toa_mean=0.0, toa_std=1.0, device="cpu")
    plan = C.ClimPlan(store.times_us)
    with pytest.raises(ValueError, match="other times"):
        C.build(store, C.ClimPlan(_us(_times()[:5])), names=feats)
    with pytest.raises(ValueError, match="wind_x_h500"):
        C.build(store, plan, names=["temperature_h500", "wind_x_h500"])
    with pytest.raises(ValueError, match="winds=True"):
        C.build(store, plan, names=feats, winds=True)
    with pytest.raises(ValueError, match="PostSpec or names"):
        C.build(store, plan)
    with pytest.raises(ValueError, match="no CPU fallback"):           # everything else in order: the device is needed
        C.build(store, plan, names=feats)


def _declared():
    text = open(os.path.join(ROOT, "include", "paradis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(paradis_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_signatures_and_library_agree_for_the_new_symbols():
    from ctypes import c_double, c_float, c_int, c_int64, c_void_p
    from paradis_model_amd import _lib
    declared = _declared()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/paradis_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is declared but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        res, args = _lib.SIGNATURES[name]
        assert res is c_int
        params = [p.strip() for p in declared[name].split(",") if p.strip() != "void"]
        want = []
        for p in params:
            kind = p.rsplit(" ", 1)[0].replace("const ", "").strip()
            want.append(c_void_p if "*" in p else {"int": c_int, "int64_t": c_int64, "float": c_float,
                                                   "double": c_double}[kind])
        assert list(args) == want, f"{name}: signature table {args} against the header's {params}"
    assert _lib.lib.paradis_abi_version() == 10
    assert _lib.lib.paradis_clim_mean_chunk() == 1024


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """rc 1 before any HIP call"""
    from paradis_model_amd import _lib
    lib = _lib.lib
    one = c_ptr = 64      # a non-NULL address that is never dereferenced: every call below is refused or does nothing
    assert lib.paradis_clim_mean(one, 0, 1, 2, 2, one, one, one, 0, 1, one, 1, one, one, None) == 1     # T = 0
    assert "bad shape" in _lib.last_error()
    assert lib.paradis_clim_mean(None, 4, 1, 2, 2, one, one, one, 0, 1, one, 1, one, one, None) == 1    # no store
    assert lib.paradis_clim_mean(one, 4, 1, 2, 2, one, None, None, 3, 1, one, 1, one, one, None) == 1   # entries, no rows
    assert lib.paradis_clim_mean(one, 4, 1, 2, 2, one, one, one, -1, 1, one, 1, one, one, None) == 1    # N < 0
    assert lib.paradis_clim_mean(one, 4, 1, 2, 2, one, one, one, 0, 0, one, 1, one, one, None) == 0     # K = 0: nothing
    assert lib.paradis_clim_mean_packed(one, None, one, 4, 1, 2, 2, one, one, one, 0, 1, one, 1, one, one, None) == 1
    units = np.array([[1, -1, 0, 1, 2, 3, 0, 0]], np.int32)
    args = lambda u, C=4, L=1: (c_ptr, c_ptr, u.ctypes.data, len(u), c_ptr, L, c_ptr, 2, C, 2, 2, None)   # noqa: E731
    assert lib.paradis_spherical_winds_inplace(*args(units, C=3)) == 1                                   # wind_z outside
    assert "outside" in _lib.last_error()
    assert lib.paradis_spherical_winds_inplace(*args(units, L=0)) == 1                                   # level outside
    twice = units.copy()
    twice[0, 4] = 1
    assert lib.paradis_spherical_winds_inplace(*args(twice)) == 1
    single = np.array([[0, 2, -1, -1, -1, -1, 0, 0]], np.int32)
    assert lib.paradis_spherical_winds_inplace(*args(single)) == 0                                       # no triple: nothing
