"""CPU checks of the forecast path (row f5): the CPU restatement tests/forecast_oracle.py against the reference's own
post-processing outputs (golden f5_post.pt), the tables ``PostSpec.from_features`` builds against the index lists the
reference found, the chunk bookkeeping against the restated predict loop (golden f5_forecast.pt), and the no-fallback
rule."""
import numpy as np
import pytest
import torch

from tests import forecast_oracle as FO
from tests._util import assert_chk, load_golden, max_rel


def _stats(g):
    return FO.channel_stats(g["names"], g["stats_seed"])


@pytest.mark.parametrize("grid", ["8x16", "9x16"])
@pytest.mark.parametrize("custom", [True, False])
def test_oracle_vs_reference_golden(grid, custom):
    g = load_golden("f5_post.pt")
    rec, names, levels = g["cases"][grid], g["names"], g["levels"]
    mean, std = _stats(g)
    x = FO.normalised_state(rec["seed"], names, 2, 1, len(names), rec["H"], rec["W"])
    assert_chk([x], rec["chk"])
    lat, lon = FO.grid_deg(rec["H"], rec["W"], rec["poles"])
    y, dew = FO.postprocess(x[:, 0], names, levels, mean, std, custom, lat, lon)
    want64, want32 = rec[f"custom{int(custom)}_f64"], rec[f"custom{int(custom)}_f32"]
    y = torch.from_numpy(y)
    for c in range(len(names)):
        e64 = max_rel(y[:, c], want64[:, c])
        spread = max_rel(want32[:, c], want64[:, c])
        assert e64 <= 2e-7, (names[c], e64)                     # same float64 expressions: one float32 rounding apart
        assert max_rel(y[:, c], want32[:, c]) <= 2e-7 + spread, names[c]
        assert spread <= 1e-6, (names[c], spread)               # the reference's own float32-grid / float64-grid spread
    assert max_rel(torch.from_numpy(dew), rec[f"dew_custom{int(custom)}"]) <= 2e-7
    # the golden's temperatures keep the vertical-velocity factor p g / (R T) finite
    assert float(want64[:, g["indices"]["temperature"]].min()) > 180.0


@pytest.mark.parametrize("custom", [True, False])
def test_postspec_tables_match_reference_indices(custom):
    from paradis_model_amd import feed
    from paradis_model_amd.config import default_config, feature_layout
    from paradis_model_amd.forecast import UNIT_LEVEL, UNIT_SINGLE, UNIT_SURFACE, PostSpec
    g = load_golden("f5_post.pt")
    names, levels, idx = g["names"], g["levels"], g["indices"]
    assert feature_layout(default_config()).output_name_order == names
    mean, std = _stats(g)
    zs = g["cases"]["8x16"][f"zscore_{custom}"]
    spec = PostSpec.from_features(None, levels, zscore_mean=mean[zs], zscore_std=std[zs], q_min=FO.Q_MIN, q_max=FO.Q_MAX,
                                  custom_normalization=custom)
    assert spec.names == names and spec.num_channels == 97 and spec.num_levels == 13
    assert (spec.it, spec.iq, spec.ix, spec.iy, spec.iz) == tuple(
        idx[v] for v in ("temperature", "specific_humidity", "wind_x", "wind_y", "wind_z"))
    assert spec.sfc == [idx["wind_x_10m"][0], idx["wind_y_10m"][0], idx["wind_z_10m"][0]]
    assert [i for i in range(97) if spec.kind[i] == feed.KIND_ZSCORE] == zs
    assert np.array_equal(spec.p0[zs], mean[zs].numpy()) and np.array_equal(spec.p1[zs], std[zs].numpy())
    hum = [i for i in range(97) if spec.kind[i] == feed.KIND_HUMIDITY]
    pre = [i for i in range(97) if spec.kind[i] == feed.KIND_PRECIP]
    assert hum == (idx["specific_humidity"] if custom else []) and len(pre) == (1 if custom else 0)
    if custom:
        assert np.all(spec.p0[hum] == np.float32(FO.Q_MIN)) and np.all(spec.p1[hum] == np.float32(FO.Q_MAX))
        assert names[pre[0]] == "total_precipitation_6hr"
    # every channel belongs to exactly one unit; levels pair the l-th index of every list with level l
    u = spec.units
    chans = sorted(int(c) for row in u for c in row[1:6] if c >= 0)
    assert chans == list(range(97))
    lev = u[u[:, 0] == UNIT_LEVEL]
    assert len(lev) == 13 and (u[:, 0] == UNIT_SURFACE).sum() == 1 and (u[:, 0] == UNIT_SINGLE).sum() == 97 - 65 - 3
    for l, row in enumerate(lev):
        assert list(row[1:7]) == [spec.iq[l], spec.it[l], spec.ix[l], spec.iy[l], spec.iz[l], l]


def test_postspec_switches_and_errors():
    from paradis_model_amd.forecast import UNIT_LEVEL, UNIT_SINGLE, PostSpec
    g = load_golden("f5_post.pt")
    names, levels = g["names"], g["levels"]
    mean, std = _stats(g)
    kw = dict(zscore_mean=mean, zscore_std=std, custom_normalization=False)
    with pytest.raises(ValueError, match="pressure levels"):
        PostSpec.from_features(names, levels[:-1], **kw)                       # 13 wind_x channels, 12 levels
    drop = [n for n in names if n != "temperature_h500"]
    keep = [i for i, n in enumerate(names) if n != "temperature_h500"]
    with pytest.raises(ValueError, match="temperature"):
        PostSpec.from_features(drop, levels, zscore_mean=mean[keep], zscore_std=std[keep], custom_normalization=False)
    with pytest.raises(ValueError, match="z-score channel"):
        PostSpec.from_features(names, levels, zscore_mean=mean[:-1], zscore_std=std[:-1], custom_normalization=False)
    with pytest.raises(ValueError, match="q_min"):
        PostSpec.from_features(names, levels, zscore_mean=mean, zscore_std=std, custom_normalization=True)
    plain = PostSpec.from_features(names, levels, winds=False, dewpoint=False, **kw)
    assert len(plain.units) == 97 and np.all(plain.units[:, 0] == UNIT_SINGLE)
    nowind = PostSpec.from_features(names, levels, winds=False, **kw)
    lv = nowind.units[nowind.units[:, 0] == UNIT_LEVEL]
    assert len(lv) == 13 and np.all(lv[:, 3:6] == -1) and np.all(lv[:, 1] >= 0) and len(nowind.units) == 13 + 97 - 26
    nodew = PostSpec.from_features(names, levels, dewpoint=False, **kw)
    lv = nodew.units[nodew.units[:, 0] == UNIT_LEVEL]
    assert np.all(lv[:, 1] == -1) and np.all(lv[:, 3:6] >= 0)
    # a level-free feature list has nothing to convert
    sfc = PostSpec.from_features(["2m_temperature", "mean_sea_level_pressure"], [], zscore_mean=[280.0, 1e5],
                                 zscore_std=[15.0, 1e3], custom_normalization=True)
    assert len(sfc.units) == 2


def test_chunk_plan_matches_restated_predict_loop():
    from paradis_model_amd.forecast import chunk_plan
    plans = load_golden("f5_forecast.pt")["plans"]
    assert set(plans) == {(1, 1, None), (5, 1, 2), (5, 2, 2), (6, 2, None), (7, 3, 1), (4, 1, 8)}
    for (S, freq, n), want in plans.items():
        plan = chunk_plan(S, freq, n)
        assert len(plan) == S
        assert FO.events_of_plan(plan) == want, (S, freq, n)
        assert FO.plan_events(S, freq, n) == want
        assert sum(p.flush[1] for p in plan if p.flush) == (S - 1) // freq + 1     # the writer's stored-step count
    with pytest.raises(ValueError):
        chunk_plan(0, 1)
    with pytest.raises(ValueError):
        chunk_plan(4, 0)


def test_rollout_golden_is_consistent():
    g = load_golden("f5_forecast.pt")["rollout"]
    tail = load_golden("f5_forecast_tail.pt")
    assert g["events"] == FO.plan_events(g["S"], g["output_frequency"], g["write_every_n"])
    assert g["start_idx"] == [0, 2] and g["n_chunks"] == 2
    assert g["chunk0"].shape == (2, 2, 97, 16, 32) and tail["chunk1"].shape == (2, 1, 97, 16, 32)


def test_forecast_entry_point_is_exported_and_refuses_cpu_tensors():
    from paradis_model_amd import _lib
    from paradis_model_amd.forecast import PostSpec, postprocess
    assert hasattr(_lib.lib, "paradis_forecast_post") and "paradis_forecast_post" in _lib.SIGNATURES
    L = _lib.lib
    # rejected before any HIP call: bad shape, batch stride shorter than a state, dew output without levels
    assert L.paradis_forecast_post(None, 0, None, 0, 0, None, 0, 0, None, None, None, 1e-12, None, 1, None, 0, None,
                                   1, 0, 8, 16, None) == 1
    assert L.paradis_forecast_post(None, 10, None, 97 * 128, 0, None, 0, 0, None, None, None, 1e-12, None, 32, None, 13,
                                   None, 1, 97, 8, 16, None) == 1
    assert "stride" in _lib.last_error()
    assert L.paradis_forecast_post(None, 512, None, 512, 0, None, 0, 0, None, None, None, 1e-12, None, 1, None, 0, None,
                                   0, 4, 8, 16, None) == 0                      # empty batch: nothing to do
    g = load_golden("f5_post.pt")
    mean, std = _stats(g)
    spec = PostSpec.from_features(g["names"], g["levels"], zscore_mean=mean, zscore_std=std, custom_normalization=False)
    lat, lon = FO.grid_deg(8, 16, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        postprocess(torch.zeros(1, 97, 8, 16), spec, lat, lon, torch.zeros(1, 1, 97, 8, 16), 0)


@pytest.mark.parametrize("custom", [True, False])
def test_kind_of_is_one_rule(custom):
    """the normalisation class of a feature is ``feed.kind_of``, for the post-processing tables and the dataset alike"""
    from types import SimpleNamespace
    from paradis_model_amd import feed
    from paradis_model_amd.config import default_config, feature_layout
    from paradis_model_amd.dataset import DeviceDataset
    from paradis_model_amd.forecast import PostSpec
    cfg = default_config()
    names = list(feature_layout(cfg).output_name_order)
    want = [feed.kind_of(f, custom) for f in names]
    assert set(want) == ({feed.KIND_ZSCORE, feed.KIND_HUMIDITY, feed.KIND_PRECIP} if custom else {feed.KIND_ZSCORE})
    n_z = want.count(feed.KIND_ZSCORE)
    spec = PostSpec.from_features(names, list(cfg.features.pressure_levels), zscore_mean=torch.zeros(n_z),
                                  zscore_std=torch.ones(n_z), q_min=FO.Q_MIN, q_max=FO.Q_MAX,
                                  custom_normalization=custom)
    assert spec.kind.tolist() == want
    stub = SimpleNamespace(custom_normalization=custom)              # no store: the method reads this attribute only
    assert [DeviceDataset._kind_of(stub, f) for f in names] == want
    assert feed.base_name("temperature_h500") == "temperature"
    assert feed.base_name("2m_temperature") == "2m_temperature" and feed.base_name("wind_x_10m") == "wind_x_10m"
