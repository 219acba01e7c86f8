"""CPU: SEEPS' definitions and host side (paradis_model_amd/seeps.py ``SeepsTable`` / ``report``,
paradis_model_amd/climatology.py ``build_seeps`` / ``SeepsClimatology``; the argument checks of csrc/seeps.hip and of
csrc/quantile.hip's SEEPS entry points).

- The scoring matrix's defining property through tests/seeps_oracle.py: under the climatological frequencies
  ``(p, 2(1-p)/3, (1-p)/3)`` every constant forecast scores 1 (within 4 double ulps: three products and two additions of
  correctly rounded terms), a perfect forecast 0.
- The oracle's climatology on hand-made cells; ``seeps.report`` on hand-made accumulators against the oracle's loops.
- The refusals of ``SeepsTable`` and ``build_seeps`` that fire before any launch; the C entry points' checks, which come
  before any HIP call; header, signature table and library agree.
- The designs of tests/seeps_cases.py meet their class conditions: cells of every class, at least half inside the bounds."""
import os
import re

import numpy as np
import pytest
import torch

from tests import seeps_cases as SC
from tests import seeps_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("paradis_clim_seeps", "paradis_clim_seeps_packed", "paradis_seeps_max_channels", "paradis_seeps_rows",
               "paradis_seeps_ws_bytes", "paradis_seeps_update")
NAMES = ["temperature_h850", "total_precipitation_24hr", "total_precipitation_6hr"]


# ---------------------------------------------------------------------------------- the definitions
@pytest.mark.parametrize("p1", [0.1, 0.4, 0.85])
def test_constant_forecasts_score_one_and_perfect_forecasts_zero(p1):
    p = float(np.float32(p1))
    M = SO.matrix(p)
    freq = [p, 2.0 * (1.0 - p) / 3.0, (1.0 - p) / 3.0]
    for cf in range(3):
        expect = sum(freq[co] * 0.5 * M[cf][co] for co in range(3))
        assert abs(expect - 1.0) <= 4 * np.finfo(np.float64).eps, (p1, cf, expect)
        assert M[cf][cf] == 0.0
    assert all(M[i][j] > 0.0 for i in range(3) for j in range(3) if i != j)


def test_oracle_climatology_on_hand_made_cells():
    nan, inf = float("nan"), float("inf")
    dry = np.float32(0.25)
    p1, thr = SO.cell_climatology(np.array([0.0, 3.0, nan, 1.0, inf, 0.1, 2.0, -0.0], np.float32), dry)
    assert p1 == np.float32(3.0 / 6.0) and thr == np.float32(2.0 + (3.0 - 2.0) * (2.0 / 3.0 * 2.0 - 1.0))
    assert SO.cell_climatology(np.array([1.0, 2.0, 3.0], np.float32), dry, 0.0)[1] == 1.0
    assert SO.cell_climatology(np.array([1.0, 2.0, 3.0], np.float32), dry, 1.0)[1] == 3.0
    p1, thr = SO.cell_climatology(np.array([0.25, 0.25, 0.25], np.float32), dry)           # == dry: strict, all wet
    assert p1 == 0.0 and thr == np.float32(0.25)
    p1, thr = SO.cell_climatology(np.array([0.0, 0.0, 0.7, 0.0], np.float32), dry)          # one wet value
    assert p1 == np.float32(0.75) and thr == np.float32(0.7)
    p1, thr = SO.cell_climatology(np.array([0.0, 0.1], np.float32), dry)                    # all dry
    assert p1 == 1.0 and np.isnan(thr)
    assert all(np.isnan(v) for v in SO.cell_climatology(np.array([nan, inf], np.float32), dry))
    assert all(np.isnan(v) for v in SO.cell_climatology(np.array([1.0, 0.0], np.float32), dry, min_count=3))
    out = SO.slot_climatology(np.arange(24, dtype=np.float32).reshape(6, 1, 2, 2), [[0, 5, 2], [], [(4, 1.0)]], [0], 9.0)
    assert out.shape == (2, 3, 1, 2, 2) and out.dtype == np.float32 and bool(np.isnan(out[:, 1]).all())
    assert np.array_equal(out[:, 0, 0, 0, 0], np.float32([2.0 / 3.0, 20.0]))               # values 0, 8, 20
    assert SO.category(0.25, 0.25, 1.0) == 1 and SO.category(1.0, 0.25, 1.0) == 2 and SO.category(0.2, 0.25, 1.0) == 0
    assert SO.cell_score(0.0, 2.0, 0.4, 1.0, 0.25, 0.1, 0.85)[1:3] == (0, 2)
    assert SO.cell_score(0.0, 2.0, 0.05, 1.0, 0.25, 0.1, 0.85) == ("masked",)
    assert SO.cell_score(0.0, nan, 0.05, 1.0, 0.25, 0.1, 0.85) == ("none",)
    assert SO.cell_score(0.0, 2.0, 0.4, 1.0, 0.25, 0.1, 0.85, slot_ok=False) == ("none",)


@pytest.mark.parametrize("grid", SC.CLIM_GRIDS)
def test_climatology_designs_meet_their_class_conditions(grid):
    x = SC.store_data(grid)
    lists = SC.hand_lists(x.shape[0], tuple(SC.SHORT), 31)
    keep = [SC.SHORT.index(n) for n in SC.DESIGN_LISTS]
    data = SO.slot_climatology(x, [lists[k] for k in keep], [SC.FEATURES.index(n) for n in SC.PICK[:2]], SC.DRY)
    for i, n in enumerate(SC.DESIGN_LISTS):
        cl = SO.classes(data[:, i], SC.P_LO, SC.P_HI)
        print(f"SEEPS design | clim {grid} | {n} entries | " + " ".join(f"{k} {int(v.sum())}" for k, v in cl.items()) +
              f" | inside {cl['inside'].mean():.3f}")
        assert all(int(v.sum()) >= 1 for v in cl.values()), (grid, n)
        assert cl["inside"].mean() >= 0.5, (grid, n)
        h, w = SC.CELL_ALL_AT_DRY
        assert bool((data[0, i, :, h, w] == 0).all()) and bool((data[1, i, :, h, w] == np.float32(SC.DRY)).all())
        h, w = SC.CELL_ONE_WET
        assert bool((data[0, i, :, h, w] == np.float32((n - 1) / n)).all())
        assert bool((data[1, i, :, h, w] == np.float32(2e-3)).all())


@pytest.mark.parametrize("name", list(SC.UPDATE_SHAPES))
def test_update_designs_meet_their_class_conditions(name):
    from paradis_model_amd import _lib
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, clim_index, chan, C = SC.update_case(name)
    cl = SO.classes(data, SC.P_LO, SC.P_HI)
    assert all(int(v.sum()) >= 1 for v in cl.values()), name
    assert cl["inside"].mean() >= 0.5, name
    real, ints, cells = SO.rows(fc, tr, data, clim_index, chan, SC.DRY, SC.P_LO, SC.P_HI)
    total = ints.sum(axis=(0, 1))
    pairs = total[:9].reshape(3, 3)
    assert bool((pairs.sum(axis=0) > 0).all()) and bool((pairs.sum(axis=1) > 0).all()) and total[9] > 0, (name, total)
    if total[:9].sum() >= 200:                                                 # every pair of categories where there is room
        assert bool((pairs > 0).all()), (name, total)
    assert int(total.sum()) < B * Cs * H * W                                   # and cells counted nowhere
    assert all(len(cells[(cs, SC.EXACT_ROW[name])]) == 1 for cs in range(Cs))
    rows = _lib.lib.paradis_seeps_rows(W)
    assert rows == max(1, 8192 // W) if W < 8192 else rows == 1
    if name == "small":
        assert W % 4 != 0 and W < 256 and H < rows and 4 < H < 8 and K == 3 and Cs == 2
        assert sorted(clim_index.tolist()) == [0, 1, 2]
    if name == "groups":
        assert W % 4 == 0 and 256 < W < 512 and W - 256 == 4 and rows == 31 and H == rows + 2
    if name == "odd":
        assert W % 2 == 1
    if name == "walks":
        assert W == 512 and H == 2


# ---------------------------------------------------------------------------------- the report
def test_report_on_hand_made_accumulators():
    from paradis_model_amd import seeps
    L, Cs, H = 3, 2, 4
    rng = np.random.default_rng(3)
    ints = rng.integers(0, 50, (L, Cs, H, 10)).astype(np.int64)
    real = rng.random((L, Cs, H, 3)) * 40.0
    n = np.array([2, 0, 5], np.int64)
    ints[2, 1, :, :9] = 0                                   # a channel with masked cells only: coverage 0, scores NaN
    real[2, 1] = 0.0
    ints[0, 1] = 0                                          # a channel that saw nothing at all: everything NaN
    real[0, 1] = 0.0
    band_w = np.array([[0.5, 1.0, 1.0, 0.5], [0.0, 0.0, 1.0, 0.5]])
    got = seeps.report(real, ints, n, band_w, ["a", "b"], ["global", "south"])
    want = SO.report(real, ints, n, band_w)
    for k, v in want.items():
        assert got[k].shape == v.shape, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(v)), k
        assert np.allclose(got[k], v, rtol=1e-12, atol=0.0, equal_nan=True), k
    assert bool(np.isnan(got["seeps"][1]).all()) and bool(np.isnan(got["coverage"][1]).all())     # never updated
    assert bool(np.isnan(got["seeps"][2, 1]).all()) and bool((got["coverage"][2, 1] == 0.0).all())
    assert bool(np.isnan(got["seeps"][0, 1]).all()) and bool(np.isnan(got["coverage"][0, 1]).all())
    # by hand: lead 0, channel 0, band 1 weighs rows 2 and 3
    N = 1.0 * ints[0, 0, 2, :9].sum() + 0.5 * ints[0, 0, 3, :9].sum()
    S = 1.0 * real[0, 0, 2].sum() + 0.5 * real[0, 0, 3].sum()
    m = 1.0 * ints[0, 0, 2, 9] + 0.5 * ints[0, 0, 3, 9]
    assert np.isclose(got["seeps"][0, 0, 1], S / N, rtol=1e-14) and np.isclose(got["coverage"][0, 0, 1], N / (N + m))
    assert np.allclose(got["seeps_skill"][0, 0], 1.0 - got["seeps"][0, 0])
    assert np.allclose(got["by_truth"][0, 0].sum(axis=-1), got["seeps"][0, 0])
    assert np.allclose(got["categories"][0, 0].sum(axis=(-1, -2)), 1.0)
    assert np.allclose(got["forecast_freq"][0, 0], got["categories"][0, 0].sum(axis=-1))
    assert np.allclose(got["truth_freq"][0, 0], got["categories"][0, 0].sum(axis=-2))
    assert got["names"] == ["a", "b"] and got["bands"] == ["global", "south"] and got["count"].tolist() == [2, 0, 5]
    text = seeps.SeepsTable.table(got, "a", "south")
    assert text.splitlines()[0] == "a / south" and "seeps_skill" in text and "d->h" in text
    with pytest.raises(ValueError, match="channel 'c'"):
        seeps.SeepsTable.table(got, "c")
    with pytest.raises(ValueError, match="band 'north'"):
        seeps.SeepsTable.table(got, "a", "north")


# ---------------------------------------------------------------------------------- the host side
def _clim(names=("total_precipitation_6hr", "total_precipitation_24hr"), K=2, H=4, W=6, dry=1e-3):
    from paradis_model_amd.climatology import SeepsClimatology
    data = torch.zeros(2, K, len(names), H, W)
    return SeepsClimatology(data, None, list(names), dry)


def test_table_refusals_before_any_launch():
    from paradis_model_amd.climatology import SeepsClimatology
    from paradis_model_amd.seeps import SeepsTable, max_channels
    lat = np.linspace(-60, 60, 4)
    cl = _clim()
    t = SeepsTable(NAMES, lat, 3, cl)
    assert t.names == cl.names and t.index == [2, 1] and t.all_names == NAMES and t.members == 1 and t.TAKES_CLIM_INDEX
    assert t.dry_threshold == float(np.float32(1e-3)) and t.p1_bounds == (float(np.float32(0.1)), float(np.float32(0.85)))
    assert tuple(t.acc_real.shape) == (3, 2, 4, 3) and t.acc_real.dtype == torch.float64
    assert tuple(t.acc_int.shape) == (3, 2, 4, 10) and t.acc_int.dtype == torch.int64 and t.n_samples.tolist() == [0] * 3
    assert t._data.data_ptr() == cl.data.data_ptr()                            # read in place
    one = SeepsTable(NAMES, lat, 1, cl, channels=["total_precipitation_24hr"])
    assert one.names == ["total_precipitation_24hr"] and one.index == [1] and tuple(one._data.shape) == (2, 2, 1, 4, 6)
    assert SeepsClimatology(cl.data, None, cl.names, 1e-3).p1.data_ptr() == cl.data[0].data_ptr()
    assert cl.threshold.data_ptr() == cl.data[1].data_ptr()
    with pytest.raises(ValueError, match="SeepsClimatology"):
        SeepsTable(NAMES, lat, 3, torch.zeros(2, 2, 2, 4, 6))
    with pytest.raises(ValueError, match="geopotential"):
        SeepsTable(NAMES, lat, 3, cl, channels=["geopotential"])
    with pytest.raises(ValueError, match="no SEEPS climatology was built for channel 'temperature_h850'"):
        SeepsTable(NAMES, lat, 3, cl, channels=["temperature_h850"])
    with pytest.raises(ValueError, match="total_precipitation_24hr"):          # the climatology's channel is no state channel
        SeepsTable(NAMES[:1] + NAMES[2:], lat, 3, cl)
    for bounds in [(0.0, 0.85), (0.1, 1.0), (0.5, 0.4), (float("nan"), 0.5), (0.1,), "ab"]:
        with pytest.raises(ValueError, match="p1_bounds"):
            SeepsTable(NAMES, lat, 3, cl, p1_bounds=bounds)
    with pytest.raises(ValueError, match="latitudes"):
        SeepsTable(NAMES, np.linspace(-60, 60, 5), 3, cl)
    with pytest.raises(ValueError, match="n_leads"):
        SeepsTable(NAMES, lat, 0, cl)
    with pytest.raises(ValueError, match="band 'x'"):
        SeepsTable(NAMES, lat, 3, cl, bands={"x": (80.0, 85.0)})
    many = [f"p{i}" for i in range(max_channels() + 1)]
    with pytest.raises(ValueError, match=f"at most {max_channels()}"):
        SeepsTable(many, lat, 3, _clim(many))
    with pytest.raises(ValueError, match="finite"):
        _clim(dry=float("inf"))
    with pytest.raises(ValueError, match=r"\[2, K, C, H, W\]"):
        SeepsClimatology(torch.zeros(3, 2, 2, 4, 6), None, cl.names, 1e-3)
    # update: the shared checks of _leadtable.py, then "no CPU fallback"
    f = torch.zeros(2, 3, 4, 6)
    idx = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="lead must be an integer in"):
        t.update(3, f, f, idx)
    with pytest.raises(ValueError, match="float32"):
        t.update(0, f.double(), f.double(), idx)
    with pytest.raises(ValueError, match="3 channels, 4 latitudes and 6 longitudes"):
        t.update(0, torch.zeros(2, 3, 4, 8), torch.zeros(2, 3, 4, 8), idx)
    with pytest.raises(ValueError, match="truth is"):
        t.update(0, f, torch.zeros(1, 3, 4, 6), idx)
    with pytest.raises(ValueError, match="dense"):
        t.update(0, torch.zeros(2, 3, 4, 12)[..., ::2], f, idx)
    with pytest.raises(ValueError, match="clim_index is needed to choose among the 2"):
        t.update(0, f, f)
    with pytest.raises(ValueError, match=r"int32 tensor \[2\]"):
        t.update(0, f, f, idx.long())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.update(0, f, f, idx)
    res = t.result()
    assert bool(np.isnan(res["seeps"]).all()) and res["seeps"].shape == (3, 2, 1) and res["categories"].shape == (3, 2, 1, 3, 3)
    cnt = t.counts()
    assert cnt["table"].shape == (3, 2, 4, 3, 3) and cnt["masked"].shape == (3, 2, 4) and cnt["sums"].shape == (3, 2, 4, 3)
    t.acc_int += 1
    t.reset()
    assert int(t.acc_int.sum()) == 0


def test_forecaster_passes_the_table_on():
    from paradis_model_amd.forecast import _passed, table_inputs
    from paradis_model_amd.seeps import SeepsTable
    t = SeepsTable(NAMES, np.linspace(-60, 60, 4), 3, _clim())
    assert _passed(None, None, None, None, seeps=t) == [t] and _passed("s", None, "e", None, None, "p", t) == ["s", "e", "p", t]
    state, truth, col = torch.zeros(2, 3, 4, 6), torch.ones(2, 3, 4, 6), torch.zeros(2, dtype=torch.int32)
    got = table_inputs(t, state, truth, col)
    assert got[0] is state and got[1].data_ptr() == truth.data_ptr() and got[2].data_ptr() == col.data_ptr()
    assert "SEEPS" in t.NOUN and "SEEPS" in t.HAS and "SEEPS" in t.NEEDS


def _cpu_store(times, feats, grid=(3, 4)):
    from paradis_model_amd.dataset import DeviceStore
    H, W = grid
    F = len(feats)
    st = {k: np.ones(F, np.float32) for k in ("mean", "std", "min", "max")}
    return DeviceStore(np.zeros((len(times), F, H, W), np.float32), times, feats, st, np.linspace(-60, 60, H),
                       np.arange(W) * (360.0 / W), np.zeros((H, W, 1), np.float32), toa_mean=0.0, toa_std=1.0,
                       device="cpu")


def test_build_seeps_refuses_on_the_host():
    from paradis_model_amd import climatology as C
    times = np.arange(np.datetime64("2020-01-01T00", "h"), np.datetime64("2020-01-03T00", "h"),
                      np.timedelta64(12, "h")).astype("datetime64[us]")
    store = _cpu_store(times, NAMES)
    plan = C.ClimPlan(store.times_us)
    ok = ["total_precipitation_6hr"]
    with pytest.raises(ValueError, match="gaussian.*unweighted"):
        C.build_seeps(store, C.ClimPlan(store.times_us, window_days=5, weights="gaussian", sigma_days=1.5), ok, 1e-3)
    with pytest.raises(ValueError, match="geopotential_h500"):
        C.build_seeps(store, plan, ok + ["geopotential_h500"], 1e-3)
    with pytest.raises(ValueError, match="other times"):
        C.build_seeps(store, C.ClimPlan(store.times_us[:3]), ok, 1e-3)
    for dry in (float("nan"), float("inf"), 1e39, "wet"):
        with pytest.raises(ValueError, match="dry_threshold"):
            C.build_seeps(store, plan, ok, dry)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="wet_level"):
            C.build_seeps(store, plan, ok, 1e-3, wet_level=q)
    with pytest.raises(ValueError, match="min_count"):
        C.build_seeps(store, plan, ok, 1e-3, min_count=0)
    with pytest.raises(ValueError, match="at least one channel"):
        C.build_seeps(store, plan, [], 1e-3)
    with pytest.raises(ValueError, match="no CPU fallback"):              # everything else in order: the device is needed
        C.build_seeps(store, plan, ok, 1e-3)
    longest = C.max_quantile_entries()
    times = (np.datetime64("2001-01-01T00", "h") + 24 * np.arange(13 * 365).astype("timedelta64[h]")) \
        .astype("datetime64[us]")
    store = _cpu_store(times, ok, grid=(1, 2))
    plan = C.ClimPlan(store.times_us, days=[40, 100], window_days=365)
    n, k = int(plan.entries.max()), int(np.argmax(plan.entries))
    assert n > longest
    with pytest.raises(ValueError, match=rf"slot {k} \(day of year {plan.days[k]}, hour 0\) has {n} entries"):
        C.build_seeps(store, plan, ok, 1e-3)


# ---------------------------------------------------------------------------------- the C ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "paradis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): (m.group(0).split("paradis_")[0], m.group(2))
            for m in re.finditer(r"\b[a-z_0-9]+\s+(paradis_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_signatures_and_library_agree_for_the_new_symbols():
    from ctypes import c_double, c_float, c_int, c_int64, c_size_t, c_void_p
    from paradis_model_amd import _lib
    declared = _declared()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/paradis_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is declared but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        res, args = _lib.SIGNATURES[name]
        assert res is (c_size_t if declared[name][0].strip() == "size_t" else c_int), name
        params = [p.strip() for p in declared[name][1].split(",") if p.strip() != "void"]
        want = []
        for p in params:
            kind = p.rsplit(" ", 1)[0].replace("const ", "").strip()
            want.append(c_void_p if "*" in p else {"int": c_int, "int64_t": c_int64, "float": c_float,
                                                   "double": c_double}[kind])
        assert list(args) == want, f"{name}: signature table {args} against the header's {params}"
    assert _lib.lib.paradis_abi_version() == 10


def test_update_entry_point_refuses_bad_arguments_without_a_gpu():
    """rc 1 before any HIP call"""
    from paradis_model_amd import _lib
    lib = _lib.lib
    one = 64      # a non-NULL address that is never dereferenced: every call below is refused or does nothing
    chan = np.array([0, 1], np.int32)
    cmax = lib.paradis_seeps_max_channels()
    assert cmax == 8 and lib.paradis_seeps_rows(0) == 0 and lib.paradis_seeps_rows(10) == 819
    assert lib.paradis_seeps_ws_bytes(3, 2, 5, 10) == 3 * 2 * 5 * (3 * 8 + 10 * 4) and lib.paradis_seeps_ws_bytes(0, 2, 5, 10) == 0

    def call(fc=one, truth=one, p1=one, thr=one, idx=one, K=2, chan_p=chan.ctypes.data, Cs=2, dry=1e-3, p_lo=0.1,
             p_hi=0.85, acc_real=one, acc_int=one, n=one, ws=one, B=2, C=3, H=4, W=6, fc_bs=72, ks=48, cs=24):
        return lib.paradis_seeps_update(fc, fc_bs, truth, 72, p1, thr, ks, cs, idx, K, chan_p, Cs, dry, p_lo, p_hi,
                                        acc_real, acc_int, n, ws, B, C, H, W, None)

    assert call(Cs=cmax + 1) == 1
    assert f"at most {cmax}" in _lib.last_error()
    assert call(Cs=0) == 1 and call(B=-1) == 1 and call(K=-1) == 1 and call(H=0) == 1
    for kw in (dict(p_lo=0.0), dict(p_lo=-0.1), dict(p_hi=1.0), dict(p_lo=0.6, p_hi=0.5), dict(p_lo=float("nan")),
               dict(p_hi=float("nan"))):
        assert call(**kw) == 1, kw
        assert "p_lo <= p_hi" in _lib.last_error()
    for dry in (float("nan"), float("inf"), -float("inf")):
        assert call(dry=dry) == 1
        assert "not finite" in _lib.last_error()
    for kw in ("fc", "truth", "p1", "thr", "idx", "chan_p"):
        assert call(**{kw: None}) == 1, kw
        assert "null input pointer" in _lib.last_error()
    for kw in ("acc_real", "acc_int", "n"):
        assert call(**{kw: None}) == 1, kw
        assert "missing" in _lib.last_error()
    assert call(ws=None) == 1
    assert "workspace" in _lib.last_error()
    assert call(fc_bs=71) == 1
    assert "batch strides" in _lib.last_error()
    assert call(cs=23) == 1
    assert "climatology strides" in _lib.last_error()
    bad = np.array([0, 3], np.int32)
    assert call(chan_p=bad.ctypes.data) == 1
    assert "channel 1 reads state channel 3" in _lib.last_error()
    assert call(B=0) == 0 and call(K=0) == 0                                                     # nothing to do
    assert call(B=0, fc=None, ws=None) == 0


def test_climatology_entry_points_refuse_bad_arguments_without_a_gpu():
    """rc 1 before any HIP call: clim_quantile's shared checks, then dry and wet_level"""
    from paradis_model_amd import _lib
    lib = _lib.lib
    one = 64

    def call(store=one, T=4, N=0, K=1, max_entries=8, C=1, dry=1e-3, wet_level=2.0 / 3.0, min_count=1, rows=one,
             out=one, flag=one):
        return lib.paradis_clim_seeps(store, T, 1, 2, 2, one, rows, N, K, max_entries, one, C, dry, wet_level, min_count,
                                      out, flag, None)

    assert call(T=0) == 1
    assert "clim_seeps: bad shape" in _lib.last_error()
    assert call(store=None) == 1
    assert "pointers required" in _lib.last_error()
    assert call(out=None) == 1 and call(flag=None) == 1
    assert call(N=3, rows=None) == 1 and call(N=-1) == 1
    assert call(max_entries=lib.paradis_clim_quantile_max_entries() + 1) == 1
    assert "max_entries" in _lib.last_error()
    assert call(min_count=0) == 1
    for dry in (float("nan"), float("inf"), -float("inf")):
        assert call(dry=dry) == 1
        assert "not finite" in _lib.last_error()
    for q in (-0.01, 1.01, float("nan")):
        assert call(wet_level=q) == 1
        assert "wet_level" in _lib.last_error()
    assert call(K=0) == 0 and call(C=0) == 0                                                     # nothing to do
    assert lib.paradis_clim_seeps_packed(one, None, one, 4, 1, 2, 2, one, one, 0, 1, 8, one, 1, 1e-3, 0.5, 1, one, one,
                                         None) == 1
    assert lib.paradis_clim_seeps_packed(one, one, one, 4, 1, 2, 2, one, one, 0, 1, 8, one, 1, float("nan"), 0.5, 1, one,
                                         one, None) == 1
    assert lib.paradis_clim_seeps_packed(one, one, one, 4, 1, 2, 2, one, one, 0, 0, 8, one, 1, 1e-3, 0.5, 1, one, one,
                                         None) == 0
