"""CPU-only checks of the store preparation (paradis_model_amd/prepare.py): the wind oracle of tests/prepare_oracle.py
against the reference's own output (tests/golden/p1_prepare.pt), the WindPlan tables, argument errors that need no
device, the new C symbols.  The kernels themselves: tests/test_hip_prepare.py."""
import os

import numpy as np
import pytest
import torch

from tests import batch_oracle as BO
from tests import prepare_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p1_prepare.pt")


def test_oracle_winds_equal_the_reference_bit_for_bit():
    gold = torch.load(GOLDEN, weights_only=False)
    assert gold["levels"] == PO.LEVELS and len(gold["winds"]) == len(PO.WIND_GRIDS)
    for (H, W, poles) in PO.WIND_GRIDS:
        rec = gold["winds"][f"{H}x{W}"]
        f = PO.wind_fields(rec["seed"], PO.WIND_T, len(PO.LEVELS), H, W)
        assert rec["chk"] == [float(sum(np.abs(a.astype(np.float64)).sum() for a in f.values()))]
        lat, lon = PO.grid_deg(H, W, poles)
        val, mag = PO.cartesian_wind(lat, lon, PO.LEVELS, f)
        for key, v, m in zip(("x", "y", "z", "x10", "y10", "z10"), val, mag):
            want = rec[key].numpy()
            assert v.dtype == np.float64 and want.dtype == np.float32 and v.shape == want.shape
            assert np.array_equal(v.astype(np.float32).view(np.int32), want.view(np.int32)), key
            assert (m >= np.abs(v)).all()


def test_oracle_statistics_on_a_known_store():
    x = np.array([[1.0, np.nan], [3.0, np.nan], [8.0, np.nan]], np.float32).reshape(3, 2, 1, 1)
    x = np.concatenate([x, x[:, :, :, :1] + 1], axis=3)                       # feature 0: 1 2 | 3 4 | 8 9
    st = PO.statistics(x, (1, 2))
    assert st["count"].tolist() == [6, 0]
    assert st["mean"][0] == np.float32(4.5) and np.isnan(st["mean"][1]) and np.isnan(st["min"][1])
    assert st["std"][0] == np.float32(np.sqrt(np.mean((np.array([1, 2, 3, 4, 8, 9.0]) - 4.5) ** 2)))
    assert (st["min"][0], st["max"][0]) == (1.0, 9.0)
    t1, t2 = st["tendencies"][1], st["tendencies"][2]
    assert t1["n_samples"] == 2 and t1["count"].tolist() == [4, 0] and t1["tendency_mean"][0] == np.float32(3.5)
    assert t2["n_samples"] == 1 and t2["count"].tolist() == [2, 0] and t2["tendency_min"][0] == 7.0
    assert PO.ulps32(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert PO.ulps32(np.float32(np.nan), np.float32(np.nan)) == 0 and PO.ulps32(np.float32(np.nan), np.float32(0)) > 1


def test_wind_plan_tables():
    from paradis_model_amd.prepare import WIND_DTYPE, WindPlan
    src, dst = PO.wind_names(PO.LEVELS)
    plan = WindPlan(src, dst, PO.LEVELS)
    assert WIND_DTYPE.itemsize == 32 and plan.rows.dtype == WIND_DTYPE and len(plan.rows) == len(PO.LEVELS) + 1
    for i, l in enumerate(PO.LEVELS):
        r = plan.rows[i]
        assert [src[r[k]] for k in ("src_u", "src_v", "src_w", "src_t")] == [
            f"u_component_of_wind_h{l}", f"v_component_of_wind_h{l}", f"vertical_velocity_h{l}", f"temperature_h{l}"]
        assert [dst[r[k]] for k in ("dst_x", "dst_y", "dst_z")] == [f"wind_x_h{l}", f"wind_y_h{l}", f"wind_z_h{l}"]
        assert r["level_hpa"] == float(l)
    s = plan.rows[-1]
    assert (src[s["src_u"]], src[s["src_v"]], s["src_w"], s["src_t"]) == ("10m_u_component_of_wind",
                                                                         "10m_v_component_of_wind", -1, -1)
    assert [dst[s[k]] for k in ("dst_x", "dst_y", "dst_z")] == ["wind_x_10m", "wind_y_10m", "wind_z_10m"]
    # one feature list at both ends: distinct columns, so the launch may run in place
    both = src + dst
    same = WindPlan(both, both, PO.LEVELS)
    assert same.in_place_ok and same.rows["dst_x"].min() >= len(src)
    # two lists that put a destination at a column index the sources read: separate tensors only
    assert not plan.in_place_ok


@pytest.mark.parametrize("side, gone", [("source", "vertical_velocity_h850"), ("source", "10m_v_component_of_wind"),
                                        ("destination", "wind_z_h1000"), ("destination", "wind_y_10m")])
def test_wind_plan_names_the_missing_feature(side, gone):
    from paradis_model_amd.prepare import WindPlan
    src, dst = PO.wind_names(PO.LEVELS)
    src, dst = [n for n in src if n != gone], [n for n in dst if n != gone]
    with pytest.raises(ValueError, match=f"{side} feature '{gone}'"):
        WindPlan(src, dst, PO.LEVELS)


def test_store_stats_argument_errors():
    from paradis_model_amd.prepare import StoreStats, store_statistics, toa_radiation_stats
    for bad in ((0,), (1, -2)):
        with pytest.raises(ValueError, match="stride"):
            StoreStats(3, 4, 8, strides=bad)
    with pytest.raises(ValueError, match="distinct"):
        StoreStats(3, 4, 8, strides=(2, 2))
    with pytest.raises(ValueError, match="bad shape"):
        StoreStats(0, 4, 8)
    with pytest.raises(ValueError, match="at least 3 time rows"):          # nothing seen yet: no device is touched
        StoreStats(3, 4, 8, strides=(2,)).result()
    with pytest.raises(ValueError, match="HIP device"):
        StoreStats(3, 4, 8, device="cpu")
    with pytest.raises(ValueError, match="HIP device"):
        store_statistics(torch.zeros(2, 3, 4, 8))
    with pytest.raises(ValueError, match="HIP device"):
        toa_radiation_stats(np.datetime64("2020-01-01T00", "us") + np.arange(2) * np.timedelta64(1, "h"),
                            np.zeros(3), np.zeros(4), device="cpu")


def test_new_symbols_and_abi():
    from paradis_model_amd import _lib
    for name in ("paradis_store_stats", "paradis_store_stats_ws_bytes", "paradis_store_stats_piece",
                 "paradis_cartesian_winds"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.paradis_abi_version() == 10
    piece = _lib.lib.paradis_store_stats_piece()
    assert piece == 8192
    ws = _lib.lib.paradis_store_stats_ws_bytes
    assert ws(0, 6, 9, 16) == 0 and ws(7, 6, 9, 16) == 7 * 6 * 80         # a block per row: 42 workgroups
    # the partials do not grow with T x F: 58 k rows x 90 features at 32x64 stay at the target grid's size
    assert ws(58440, 90, 32, 64) <= (4096 + 90) * 80
    assert ws(8, 97, 721, 1440) == 97 * 127 * 80                           # large planes: one block of all rows per piece
    # argument checks happen before any HIP call
    lib = _lib.lib
    assert lib.paradis_store_stats(None, 4, None, 0, 2, 4, 8, -1, -1, 1, None, 1, None, None) == 1
    assert "nothing to accumulate" in _lib.last_error()
    assert lib.paradis_store_stats(None, 4, None, 0, 2, 4, 8, 0, 1, 0, None, 2, None, None) == 1
    assert "stride must be >= 1" in _lib.last_error()
    assert lib.paradis_store_stats(None, 4, None, 0, 2, 4, 8, 0, 2, 1, None, 2, None, None) == 1
    assert lib.paradis_store_stats(None, 4, None, 3, 2, 4, 8, 0, 1, 1, None, 2, None, None) == 1
    assert lib.paradis_store_stats(None, 4, None, 0, 2, 4, 8, 0, 1, 1, None, 2, None, None) == 1
    assert "null pointer" in _lib.last_error()
    assert lib.paradis_cartesian_winds(None, 4, None, 4, None, None, 1, None, 2, 4, 8, None) == 1


def test_device_store_on_the_cpu_needs_given_statistics():
    from paradis_model_amd.dataset import DeviceStore
    case = BO.build_case(4, 6, n_time_inputs=2, steps=1, n_samples=3, seed=5)
    args = (case.store.numpy(), case.times, case.features)
    grid = (case.lat, case.lon, case.constants)
    with pytest.raises(ValueError, match="statistics need the HIP device"):
        DeviceStore(*args, None, *grid, case.toa_mean, case.toa_std, device="cpu")
    with pytest.raises(ValueError, match="statistics need the HIP device"):
        DeviceStore(*args, case.stats, *grid, device="cpu")
    with pytest.raises(ValueError, match="statistics need the HIP device"):
        DeviceStore(*args, case.stats, *grid, case.toa_mean, None, device="cpu")
    store = DeviceStore(*args, case.stats, *grid, case.toa_mean, case.toa_std, device="cpu")      # as before
    assert store.toa_mean == float(case.toa_mean) and set(store.stats) == {"mean", "std", "min", "max"}
