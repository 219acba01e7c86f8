"""GPU: the store preparation (paradis_model_amd/prepare.py, csrc/prepare.hip) against the fp64 numpy oracle of
tests/prepare_oracle.py and the reference's own outputs (tests/golden/p1_prepare.pt).

Statistics at T = 7, F = 6.  A workgroup owns one piece of PLANE_PIECE = 8192 cells of one feature's plane over a block
of time rows; a row of quads is 1024 cells:
  (9, 16)    144 cells: a partial row of quads, 16-byte path
  (9, 15)    135 cells: planes 4-byte aligned only, scalar path, a last quad of three cells
  (33, 64)   2112 cells: two full rows of quads and 64 cells
  (65, 128)  8320 cells: one whole piece plus a tail piece of 128
Bounds: counts exact; min / max bit-exact; mean and std within 1 float32 ulp of the oracle's float32 - the double sums
about the pivot are good to about 1e-13, so only the final rounding can differ.  Winds: 1 float32 ulp of the value plus
2^-40 of the summed magnitudes of its terms (double arithmetic's slack where the terms cancel).  TOA: 1e-5 of the
largest radiation value, the per-value bound tests/test_hip_feed.py grants this channel (a mean or an rms of errors
cannot exceed it)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import batch_oracle as BO
from tests import prepare_oracle as PO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p1_prepare.pt")
T, F = 7, 6
GRIDS = [(9, 16), (9, 15), (33, 64), (65, 128)]
STRIDES = (1, 2, 6)


def test_shapes_sit_on_the_kernel_piece():
    from paradis_model_amd import _lib
    piece = _lib.lib.paradis_store_stats_piece()
    sizes = [h * w for h, w in GRIDS]
    assert any(s % 4 for s in sizes) and any(s < 1024 and s % 4 == 0 for s in sizes)
    assert any(1024 < s < piece and s % 1024 for s in sizes) and any(piece < s < 2 * piece for s in sizes)


@functools.lru_cache(maxsize=None)
def _store(grid):
    x = PO.stats_store(900 + GRIDS.index(grid), T, *grid)
    return x, PO.statistics(x, STRIDES)            # computed once, shared, never written


@functools.lru_cache(maxsize=None)
def _gold():
    return torch.load(GOLDEN, weights_only=False)


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def _check_five(got, want, prefix, what):
    assert got["count"].dtype == np.int64 and np.array_equal(got["count"], want["count"]), (what, "count")
    for key in ("min", "max"):
        g, w = got[prefix + key], want[prefix + key]
        assert g.dtype == np.float32 and g.shape == (F,)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(_bits(g)[~np.isnan(w)], _bits(w)[~np.isnan(w)]), \
            (what, key, g, w)
    for key in ("mean", "std"):
        g, w = got[prefix + key], want[prefix + key]
        assert g.dtype == np.float32 and g.shape == (F,)
        u = PO.ulps32(g, w)
        print(f"{what} {prefix}{key}: ulps {u.tolist()}")
        assert (u <= 1).all(), (what, key, u, g, w)
    for key in ("mean", "std", "min", "max"):                       # the feature that is NaN everywhere
        assert np.isnan(got[prefix + key][5])
        assert not np.isnan(got[prefix + key][:5]).any()


def _check(got, want, strides, what):
    _check_five(got, want, "", what)
    assert sorted(got["tendencies"]) == sorted(strides)
    for s in strides:
        g, w = got["tendencies"][s], want["tendencies"][s]
        assert g["n_samples"] == w["n_samples"] == T - s
        _check_five(g, w, "tendency_", f"{what} stride {s}")


@pytest.mark.parametrize("grid", GRIDS)
def test_statistics_against_oracle(grid):
    from paradis_model_amd.prepare import store_statistics
    x, want = _store(grid)
    got = store_statistics(torch.from_numpy(x).cuda(), STRIDES)
    _check(got, want, STRIDES, f"{grid}")
    assert want["count"].tolist() == [T * grid[0] * grid[1]] * 4 + [T * grid[0] * grid[1] - 1 - grid[1], 0]


def test_field_alone_and_single_strides():
    """the three launch variants: field alone, field + tendency, tendency alone (every stride after the first)"""
    from paradis_model_amd.prepare import store_statistics
    x, want = _store((33, 64))
    xd = torch.from_numpy(x).cuda()
    alone = store_statistics(xd)
    assert alone["tendencies"] == {}
    _check_five(alone, want, "", "field alone")
    for order in ((6, 1), (2,)):
        _check(store_statistics(xd, order), want, order, f"strides {order}")


def test_stride_past_the_store_raises():
    from paradis_model_amd.prepare import StoreStats, store_statistics
    x, _ = _store((9, 16))
    with pytest.raises(ValueError, match="at least 8 time rows"):
        store_statistics(torch.from_numpy(x).cuda(), (7,))
    st = StoreStats(F, 9, 16, strides=(1, 7))
    st.update(torch.from_numpy(x).cuda())
    with pytest.raises(ValueError, match="stride 7"):
        st.result()


def _streamed(x, rows, strides, numpy_slabs=False):
    from paradis_model_amd.prepare import StoreStats
    st = StoreStats(F, x.shape[2], x.shape[3], strides)
    xd = torch.from_numpy(x).cuda()
    for a in range(0, x.shape[0], rows):
        st.update(x[a:a + rows] if numpy_slabs else xd[a:a + rows])
    return st


@pytest.mark.parametrize("rows", [1, 3, 7])
@pytest.mark.parametrize("grid", GRIDS)
def test_streaming_in_slabs(grid, rows):
    """slabs of 1 row are shorter than the stride: the pair's earlier row comes from the rows kept"""
    x, want = _store(grid)
    strides = (1, 2)
    st = _streamed(x, rows, strides, numpy_slabs=(rows == 3))
    assert st.rows_seen == T
    got = st.result()
    _check(got, want, strides, f"{grid} slabs of {rows}")
    one = _streamed(x, T, strides).result()
    assert np.array_equal(got["count"], one["count"])
    for s in strides:
        assert got["tendencies"][s]["n_samples"] == one["tendencies"][s]["n_samples"]
        assert np.array_equal(got["tendencies"][s]["count"], one["tendencies"][s]["count"])


def test_two_runs_are_bit_identical():
    x, _ = _store((65, 128))
    a, b = _streamed(x, 3, (1, 2)), _streamed(x, 3, (1, 2))
    assert torch.equal(a._acc.view(torch.int64), b._acc.view(torch.int64))
    ra, rb = a.result(), b.result()
    for key in ("mean", "std", "min", "max"):
        assert np.array_equal(_bits(ra[key]), _bits(rb[key]))


@pytest.mark.parametrize("grid", [(9, 16), (33, 64), (65, 128)])
def test_scalar_loads_give_the_same_bits(grid):
    """the same store at a base that is 4-byte aligned only takes the scalar path of load_quad"""
    from paradis_model_amd.prepare import StoreStats
    x, _ = _store(grid)
    xd = torch.from_numpy(x).cuda()
    buf = torch.empty(xd.numel() + 1, device="cuda")
    off = buf[1:].view(xd.shape).copy_(xd)
    assert xd.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.is_contiguous()
    accs = []
    for t in (xd, off):
        st = StoreStats(F, *grid, strides=(1, 2))
        st.update(t[:4])
        st.update(t[4:])
        accs.append(st._acc.view(torch.int64))
    assert torch.equal(accs[0], accs[1])


# ------------------------------------------------------------------------------------------------- winds
def _wind_bound(want64, mag):
    return np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64) + 2.0 ** -40 * mag


def _check_winds(dst, dst_names, levels, want, mag, what):
    col = {n: j for j, n in enumerate(dst_names)}
    x, y, z, x10, y10, z10 = want
    mx, my, mz, mx10, my10, mz10 = mag
    for i, l in enumerate(levels):
        for a, w, m in (("x", x, mx), ("y", y, my), ("z", z, mz)):
            err = np.abs(dst[:, col[f"wind_{a}_h{l}"]].astype(np.float64) - w[:, i])
            assert (err <= _wind_bound(w[:, i], m[:, i])).all(), (what, a, l, err.max())
    for a, w, m in (("x", x10, mx10), ("y", y10, my10), ("z", z10, mz10)):
        err = np.abs(dst[:, col[f"wind_{a}_10m"]].astype(np.float64) - w)
        assert (err <= _wind_bound(w, m)).all(), (what, a, "10m", err.max())


@pytest.mark.parametrize("grid", PO.WIND_GRIDS)
def test_winds_against_the_reference(grid):
    from paradis_model_amd.prepare import WindPlan, cartesian_winds
    H, W, poles = grid
    rec = _gold()["winds"][f"{H}x{W}"]
    levels = _gold()["levels"]
    f = PO.wind_fields(rec["seed"], PO.WIND_T, len(levels), H, W)
    lat, lon = PO.grid_deg(H, W, poles)
    src_names, dst_names = PO.wind_names(levels)
    src = PO.pack_sources(src_names, levels, f)
    g = np.random.default_rng(5)
    dst0 = g.normal(0, 1, (PO.WIND_T, len(dst_names), H, W)).astype(np.float32)
    sd, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst0).cuda()
    plan = WindPlan(src_names, dst_names, levels)
    assert cartesian_winds(sd, dd, plan, lat, lon) is dd
    got = dd.cpu().numpy()
    want = tuple(rec[k].numpy().astype(np.float64) for k in ("x", "y", "z", "x10", "y10", "z10"))
    _, mag = PO.cartesian_wind(lat, lon, levels, f)
    _check_winds(got, dst_names, levels, want, mag, f"{H}x{W}")
    # what the plan does not name is untouched, bit for bit
    j = dst_names.index("2m_temperature")
    assert np.array_equal(got[:, j].view(np.int32), dst0[:, j].view(np.int32))
    assert np.array_equal(sd.cpu().numpy().view(np.int32), src.view(np.int32))
    with pytest.raises(ValueError, match="also a source column"):
        cartesian_winds(sd, sd, WindPlan(src_names, src_names[:1] + dst_names[:12] + src_names[13:], levels), lat, lon)


def test_winds_in_place():
    """33x64 (two blocks on the 16-byte path), the raw fields and the winds side by side in one tensor"""
    from paradis_model_amd.prepare import WindPlan, cartesian_winds
    H, W, levels = 33, 64, PO.LEVELS
    f = PO.wind_fields(711, PO.WIND_T, len(levels), H, W)
    lat, lon = PO.grid_deg(H, W, True)
    src_names, dst_names = PO.wind_names(levels)
    names = src_names + dst_names
    before = PO.pack_sources(names, levels, f)
    both = torch.from_numpy(before).cuda()
    cartesian_winds(both, both, WindPlan(names, names, levels), lat.astype(np.float32).astype(np.float64), lon)
    got = both.cpu().numpy()
    want, mag = PO.cartesian_wind(lat.astype(np.float32), lon, levels, f)
    _check_winds(got, names, levels, want, mag, "in place")
    keep = [j for j, n in enumerate(names) if not n.startswith("wind_")]
    assert len(keep) == len(src_names) + 1
    assert np.array_equal(got[:, keep].view(np.int32), before[:, keep].view(np.int32))


# ------------------------------------------------------------------------------------------------- TOA, DeviceStore
def test_toa_radiation_stats_against_the_reference():
    from paradis_model_amd.prepare import toa_radiation_stats
    toa = _gold()["toa"]
    H, W, poles = toa["grid"]
    lat, lon = PO.grid_deg(H, W, poles)
    times = np.datetime64(toa["t0"], "us") + np.arange(toa["n_times"]) * np.timedelta64(1, "h")
    assert len(toa["cases"]) == 2
    for case in toa["cases"]:
        mean, std = toa_radiation_stats(times, lat, lon, *case["strides"])
        assert isinstance(mean, float) and isinstance(std, float)
        bound = 1e-5 * case["max"]
        print(f"toa {case['strides']}: mean {mean} vs {case['mean']}, std {std} vs {case['std']}, bound {bound}")
        assert case["max"] > 1e6 and case["std"] > 0
        assert abs(mean - case["mean"]) <= bound and abs(std - case["std"]) <= bound


def test_device_store_computes_its_statistics():
    from paradis_model_amd.dataset import DeviceDataset, DeviceStore
    from paradis_model_amd.prepare import store_statistics, toa_radiation_stats
    case = BO.build_case(9, 16, n_time_inputs=2, interval_steps=1, delta_steps=1, steps=2, n_samples=4, base=1, seed=41)
    args = (case.store.numpy(), case.times, case.features)
    grid = (case.lat, case.lon, case.constants)
    auto = DeviceStore(*args, None, *grid, device="cuda")
    want = store_statistics(auto.data)
    assert sorted(auto.stats) == ["max", "mean", "min", "std"]
    for key, v in auto.stats.items():
        assert v.dtype == np.float32 and np.array_equal(_bits(v), _bits(want[key])) and np.isfinite(v).all()
    oracle = PO.statistics(case.store.numpy())
    for key in ("mean", "std"):
        assert (PO.ulps32(auto.stats[key], oracle[key]) <= 1).all()
    assert (auto.toa_mean, auto.toa_std) == toa_radiation_stats(case.times, case.lat, case.lon)
    assert auto.toa_std > 0
    given = DeviceStore(*args, auto.stats, *grid, auto.toa_mean, auto.toa_std, device="cuda")
    half = DeviceStore(*args, auto.stats, *grid, toa_mean=3.5, device="cuda")       # one TOA value given, one computed
    assert (half.toa_mean, half.toa_std) == (3.5, auto.toa_std)
    idx = [2, 0, 3]
    batches = [DeviceDataset(s, case.cfg, case.start_date, case.end_date, case.steps).batch(idx) for s in (auto, given)]
    for a, b in zip(*batches):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t).all() for t in batches[0])
