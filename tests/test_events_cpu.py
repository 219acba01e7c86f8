"""Host side of the event verification, no GPU: the ``scores`` formulas against exact fractions, the numpy oracle's own
closed forms (tests/events_oracle.py), the argument checks and host arithmetic of ``events.EventTable`` on
``device="cpu"``, the ``Forecaster.run(events=...)`` refusals and the C ABI's refusals before any HIP call."""
import ctypes
import math
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

from paradis_model_amd import events as EV
from tests import events_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tp", "u10", "v10", "t2m"]
LAT = np.linspace(-80.0, 80.0, 5)
SYMBOLS = ("paradis_events_max_thresholds", "paradis_events_rows", "paradis_events_ws_bytes", "paradis_events_update")
A, B_, C_, D = 28, 72, 23, 2680            # the known-answer table: hits, false alarms, misses, correct negatives


def plain(c0, thr, direction="ge"):
    return {"kind": "plain", "c0": c0, "thresholds": list(thr), "direction": direction}


# ================================================================================================ 1. scores
def test_scores_known_answer():
    a, b, c, d = (Fraction(v) for v in (A, B_, C_, D))
    n = a + b + c + d
    ar = (a + b) * (a + c) / n
    pod, pofd = a / (a + c), b / (b + d)
    want = {"pod": Fraction(28, 51), "far": Fraction(72, 100), "csi": Fraction(28, 123),
            "frequency_bias": Fraction(100, 51), "pofd": pofd, "base_rate": (a + c) / n,
            "ets": (a - ar) / (a + b + c - ar), "hss": 2 * (a * d - b * c) / ((a + c) * (c + d) + (a + b) * (b + d))}
    assert pod == want["pod"]
    lf, lh, l1f, l1h = (math.log(float(v)) for v in (pofd, pod, 1 - pofd, 1 - pod))
    want["sedi"] = (lf - lh - l1f + l1h) / (lf + lh + l1f + l1h)
    got = EV.scores(A, B_, C_, D)
    assert set(got) == set(EV.SCORES) == set(want)
    for k, v in want.items():
        assert got[k].dtype == np.float64 and got[k].shape == ()
        assert abs(float(got[k]) - float(v)) <= 1e-15 * abs(float(v)), (k, float(got[k]), float(v))
    assert EV.EventTable.scores is EV.scores


def test_scores_zero_denominators_are_nan_without_warnings():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        z = EV.scores(0, 0, 0, 0)
        assert all(np.isnan(z[k]) for k in EV.SCORES)
        none_observed = EV.scores(0, 5, 0, 10)          # a + c = 0
        assert np.isnan(none_observed["pod"]) and np.isnan(none_observed["frequency_bias"])
        assert none_observed["far"] == 1.0 and none_observed["csi"] == 0.0 and np.isnan(none_observed["sedi"])
        perfect = EV.scores(7, 0, 0, 20)                # pofd = 0, pod = 1: ln 0
        assert perfect["pod"] == 1.0 and perfect["far"] == 0.0 and perfect["ets"] == 1.0 and perfect["hss"] == 1.0
        assert np.isnan(perfect["sedi"])
        arr = EV.scores(np.array([A, 0]), np.array([B_, 0]), np.array([C_, 0]), np.array([D, 0]))
        assert arr["csi"].shape == (2,) and arr["csi"][0] == 28 / 123 and np.isnan(arr["csi"][1])


# ================================================================================================ 2. the oracle itself
def known_row_fields(W=A + B_ + C_ + D):
    """one row [1, 1, 1, W] whose cells are, for threshold 1.0: A hits, B_ false alarms, C_ misses, D correct negatives"""
    f = np.zeros((1, 1, 1, W), np.float32)
    t = np.zeros((1, 1, 1, W), np.float32)
    f[..., :A + B_] = 2.0
    t[..., :A] = 2.0
    t[..., A + B_:A + B_ + C_] = 2.0
    return f, t


def test_oracle_known_table_row():
    f, t = known_row_fields()
    cnt = EO.counts(f, t, [plain(0, [1.0])])
    assert cnt["ambiguous"] == 0
    assert cnt["valid"].tolist() == [[A + B_ + C_ + D]]
    assert (cnt["forecast_yes"][0, 0, 0], cnt["observed_yes"][0, 0, 0], cnt["both"][0, 0, 0]) == (A + B_, A + C_, A)
    a, b, c, d = EO.tables(cnt, np.array([[0.5]]))
    assert (a[0, 0, 0], b[0, 0, 0], c[0, 0, 0], d[0, 0, 0]) == (A / 2, B_ / 2, C_ / 2, D / 2)


def test_oracle_le_is_ge_on_negated_data_and_ties_count_both_ways():
    rng = np.random.default_rng(3)
    f = rng.standard_normal((2, 1, 3, 17)).astype(np.float32)
    t = rng.standard_normal((2, 1, 3, 17)).astype(np.float32)
    f[0, 0, 1, 4] = t[1, 0, 2, 0] = np.float32(0.25)                      # exact ties
    ge = EO.counts(-f, -t, [plain(0, [-0.25, 0.5], "ge")])
    le = EO.counts(f, t, [plain(0, [0.25, -0.5], "le")])
    for k in ("valid", "forecast_yes", "observed_yes", "both"):
        assert np.array_equal(ge[k], le[k]), k
    one = np.full((1, 1, 1, 1), 0.25, np.float32)
    for direction in ("ge", "le"):
        cnt = EO.counts(one, one, [plain(0, [0.25], direction)])
        assert cnt["both"][0, 0, 0] == 1 and cnt["ambiguous"] == 0


def test_oracle_negative_zero_is_an_event_at_zero():
    f = np.array([-0.0, 0.0, -1e-30], np.float32).reshape(1, 1, 1, 3)
    cnt = EO.counts(f, f, [plain(0, [0.0], "ge"), plain(0, [0.0], "le"), plain(0, [-0.0], "ge")])
    assert cnt["both"][:, 0, 0].tolist() == [2, 3, 2]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_oracle_non_finite_cells_leave_every_class(bad):
    rng = np.random.default_rng(5)
    f = rng.standard_normal((1, 2, 2, 9)).astype(np.float32)
    t = rng.standard_normal((1, 2, 2, 9)).astype(np.float32)
    clim = np.zeros((1, 2, 2, 9), np.float32)
    srcs = [plain(0, [-10.0]), {"kind": "speed", "c0": 0, "c1": 1, "thresholds": [0.0], "direction": "ge"},
            {"kind": "anomaly", "c0": 0, "thresholds": [-10.0], "direction": "ge"}]
    full = EO.counts(f, t, srcs, clim)
    assert (full["both"][:, :, 0] == 9).all() and (full["valid"] == 9).all()     # every cell an event in both
    for where in ("forecast", "truth", "clim"):
        f2, t2, c2 = f.copy(), t.copy(), clim.copy()
        {"forecast": f2, "truth": t2, "clim": c2}[where][0, 0, 1, 3] = bad
        cnt = EO.counts(f2, t2, srcs, c2)
        hit = [0, 1, 2] if where != "clim" else [2]                      # channel 0 feeds all three sources
        for s in range(3):
            want = np.array([9, 8 if s in hit else 9])
            for k in ("valid",):
                assert np.array_equal(cnt[k][s], want), (where, s)
            for k in ("forecast_yes", "observed_yes", "both"):
                assert np.array_equal(cnt[k][s, :, 0], want), (where, s, k)
    f2 = f.copy()
    f2[0, 1, 0, 0] = bad                                                 # the speed's second component only
    cnt = EO.counts(f2, t, srcs, clim)
    assert cnt["valid"][:, 0].tolist() == [9, 8, 9]


def test_oracle_speed_tie_and_bad_slot():
    f = np.zeros((2, 2, 1, 2), np.float32)
    f[:, 0], f[:, 1] = 3.0, 4.0
    f[1, 0, 0, 1] = 2.0
    speed = {"kind": "speed", "c0": 0, "c1": 1, "thresholds": [5.0], "direction": "ge"}
    cnt = EO.counts(f, f, [speed, dict(speed, direction="le")])
    assert cnt["both"][:, 0, 0].tolist() == [3, 4] and cnt["ambiguous"] == 0
    near = f.copy()
    near[0, 0, 0, 0] = np.nextafter(np.float32(3.0), np.float32(4.0))
    assert EO.counts(near, f, [speed])["ambiguous"] == 1
    clim = np.ones((2, 2, 1, 2), np.float32)
    anom = {"kind": "anomaly", "c0": 0, "thresholds": [1.5], "direction": "ge"}
    cnt = EO.counts(f, f, [anom, plain(0, [2.5])], clim, np.array([1, 2]))       # sample 1: slot out of range
    assert cnt["valid"].tolist() == [[2], [4]] and cnt["both"][:, 0, 0].tolist() == [2, 3]


# ================================================================================================ 3. EventTable on the host
EVENTS = {"rain": {"source": "tp", "thresholds": [1.0, 5.0, 0.2], "direction": "ge"},
          "gale": {"source": ("speed", "u10", "v10"), "thresholds": [17.2]},
          "cold": {"source": ("anomaly", "t2m"), "thresholds": [-5.0, -10.0], "direction": "le"}}


def _table(**kw):
    kw.setdefault("climatology", torch.zeros(2, 4, 5, 8))
    kw.setdefault("bands", {"nh": (20, 90), "all": (-90, 90)})
    return EV.EventTable(NAMES, LAT, 2, kw.pop("events", EVENTS), device="cpu", **kw)


def test_event_table_tables_and_shapes():
    e = _table()
    tmax = EV.max_thresholds()
    assert tmax == 8 and e.labels == ["rain", "gale", "cold"] and e.T == 3 and e.n_thresholds == [3, 1, 2]
    assert e.acc.shape == (2, 3, 5, 1 + 3 * tmax) and e.acc.dtype == torch.int64 and e.n_samples.dtype == torch.int64
    assert e._src.tolist() == [[0, 0, 0, 3], [1, 1, 2, 1], [2, 3, 0, 2]]
    assert e._thr[0, :4].tolist() == [1.0, 1.0, 5.0, np.float32(0.2)]
    assert e._thr[2, :3].tolist() == [-1.0, 5.0, 10.0]                    # "le": sign -1 and the negated thresholds
    assert e.thresholds[2] == [-5.0, -10.0] and e.directions == ["ge", "ge", "le"]
    assert e.band_w.shape == (2, 5) and e.band_w[0, :3].tolist() == [0.0, 0.0, 0.0]
    # 35 MB at 721 rows, 6 sources, 40 leads
    assert 40 * 6 * 721 * (1 + 3 * tmax) * 8 == 34_608_000


def test_event_table_constructor_errors():
    def bad(match, events=None, **kw):
        with pytest.raises(ValueError, match=match):
            _table(events=EVENTS if events is None else events, **kw)

    ok = {"source": "tp", "thresholds": [1.0]}
    bad("not among the names", {"x": {"source": "q700", "thresholds": [1.0]}})
    bad("not among the names", {"x": {"source": ("speed", "u10", "w10"), "thresholds": [1.0]}})
    bad("with itself", {"x": {"source": ("speed", "u10", "u10"), "thresholds": [1.0]}})
    bad("source must be", {"x": {"source": ("speed", "u10"), "thresholds": [1.0]}})
    bad("source must be", {"x": {"source": ("gust", "u10", "v10"), "thresholds": [1.0]}})
    bad("9 thresholds", {"x": {"source": "tp", "thresholds": list(range(EV.max_thresholds() + 1))}})
    bad("0 thresholds", {"x": {"source": "tp", "thresholds": []}})
    for v in (np.nan, np.inf, 1e39):
        bad("finite", {"x": {"source": "tp", "thresholds": [1.0, v]}})
    bad("list of numbers", {"x": {"source": "tp", "thresholds": ["wet"]}})
    bad("direction", {"x": dict(ok, direction="gt")})
    bad("must be a dict", {"x": dict(ok, threshold=1.0)})
    bad("must be a dict", {"x": [1.0]})
    bad("non-empty dict", {})
    bad("at most", {f"e{i}": ok for i in range(17)})
    with pytest.raises(ValueError, match="no climatology"):
        _table(climatology=None)
    assert _table(climatology=None, events={"rain": EVENTS["rain"]}).climatology is None
    bad("climatology must be", climatology=torch.zeros(2, 3, 5, 8))
    bad("climatology must be", climatology=torch.zeros(2, 4, 5, 8, dtype=torch.float64))
    bad("EventTable: band 'x'", bands={"x": (10, -10)})
    bad("EventTable: band 'x'", bands={"x": (81, 90)})                     # holds no row
    bad("bands must be", bands={})
    bad("weights", weights=torch.ones(4))
    bad("weights", weights=-torch.ones(5))
    for n_leads in (0, 1.5, True):
        with pytest.raises(ValueError, match="n_leads"):
            EV.EventTable(NAMES, LAT, n_leads, {"r": ok}, device="cpu")
    with pytest.raises(ValueError, match="lat_deg"):
        EV.EventTable(NAMES, [0.0, 91.0], 1, {"r": ok}, device="cpu")
    poles = EV.EventTable(NAMES, [-90.0, 0.0, 90.0], 1, {"r": ok}, device="cpu")
    assert poles.band_w.tolist() == [[0.0, 1.0, 0.0]]


def test_event_table_update_argument_errors_on_cpu_tensors():
    e = _table()
    f = torch.zeros(2, 4, 5, 8)
    k = torch.zeros(2, dtype=torch.int32)

    def bad(match, lead=0, fc=f, truth=f, idx=k, exc=ValueError, table=e):
        with pytest.raises(exc, match=match):
            table.update(lead, fc, truth, idx)

    bad("lead", lead=2)
    bad("lead", lead=True)
    bad("float32", fc=f.double())
    bad(r"\[B, C, H, W\]", truth=f[0])
    bad("channels", fc=torch.zeros(2, 3, 5, 8), truth=torch.zeros(2, 3, 5, 8))
    bad("truth is", truth=torch.zeros(1, 4, 5, 8))
    bad("dense", fc=torch.zeros(2, 4, 5, 16)[..., ::2])
    bad("longitudes", fc=torch.zeros(2, 4, 5, 6), truth=torch.zeros(2, 4, 5, 6))
    bad("clim_index is needed", idx=None)
    bad("int32", idx=k.long())
    bad("int32", idx=torch.zeros(3, dtype=torch.int32))
    bad("no climatology", table=_table(climatology=None, events={"rain": EVENTS["rain"]}))
    bad("MI355X", exc=RuntimeError)                                      # every host check passed: the device check
    e.bind(8)
    with pytest.raises(ValueError, match="bound"):
        e.bind(16)


def _filled():
    """a table whose accumulator is filled by hand with the oracle's rows of two updates at lead 0"""
    e = _table()
    rng = np.random.default_rng(7)
    srcs = [plain(0, [1.0, 5.0, 0.2]), {"kind": "speed", "c0": 1, "c1": 2, "thresholds": [17.2], "direction": "ge"},
            {"kind": "anomaly", "c0": 3, "thresholds": [-5.0, -10.0], "direction": "le"}]
    clim = rng.standard_normal((2, 4, 5, 8)).astype(np.float32)
    total = None
    for B in (2, 3):
        t = (rng.standard_normal((B, 4, 5, 8)) * 8).astype(np.float32)
        f = (t + rng.standard_normal((B, 4, 5, 8)) * 4).astype(np.float32)
        f[0, 0, 2, 1] = np.nan
        total = EO.add_counts(total, EO.counts(f, t, srcs, clim, rng.integers(0, 2, B)))
    TM = EV.max_thresholds()
    acc = np.zeros(tuple(e.acc.shape), np.int64)
    acc[0, :, :, 0] = total["valid"]
    for s, n in enumerate(e.n_thresholds):
        acc[0, s, :, 1:1 + n] = total["forecast_yes"][s, :, :n]
        acc[0, s, :, 1 + TM:1 + TM + n] = total["observed_yes"][s, :, :n]
        acc[0, s, :, 1 + 2 * TM:1 + 2 * TM + n] = total["both"][s, :, :n]
    e.acc.copy_(torch.from_numpy(acc))
    e.n_samples[0] = 5
    e.bind(8)
    return e, total


def test_event_table_result_from_a_hand_filled_accumulator():
    e, total = _filled()
    cnt = e.counts()
    for k in ("valid", "forecast_yes", "observed_yes", "both"):
        assert cnt[k].dtype == np.int64 and np.array_equal(cnt[k][0], total[k]), k
    assert (cnt["both"][0, 1, :, 1:] == -1).all() and (cnt["both"][0, 2, :, 2:] == -1).all()
    assert cnt["n_samples"].tolist() == [5, 0]
    res = e.result()
    want = dict(zip(EV.TABLES, EO.tables(total, e.band_w)))
    want.update(EV.scores(*(want[k] for k in EV.TABLES)))
    # all terms are non-negative: the float64 sum of H products is within (H + 1) 2^-53 < 1e-13 of exact in any order
    for k in EV.TABLES:
        got = res[k]
        assert got.shape == (2, 3, 2, 3) and got.dtype == np.float64, k
        assert np.array_equal(np.isnan(got[0]), np.isnan(want[k])), k
        fin = np.isfinite(want[k])
        assert np.all(np.abs(got[0][fin] - want[k][fin]) <= 1e-12 * np.abs(want[k][fin])), k
        assert np.isnan(got[1]).all(), k                                 # a lead never updated
    again = EV.scores(*(res[k] for k in EV.TABLES))                      # the scores are `scores` of those tables
    for k in EV.SCORES:
        assert res[k].shape == (2, 3, 2, 3) and np.array_equal(res[k], again[k], equal_nan=True), k
        assert np.isfinite(res[k][0, 0]).all() and np.isnan(res[k][1]).all(), k
        near = np.isfinite(want[k])
        assert np.allclose(res[k][0][near], want[k][near], rtol=1e-9, atol=0), k
    assert np.isnan(res["hits"][0, 1, :, 1:]).all() and np.isfinite(res["hits"][0, 0]).all()
    n = sum(res[k] for k in EV.TABLES)[0, 0, :, 0]
    assert np.allclose(n, (e.band_w * total["valid"][0][None, :]).sum(axis=1), rtol=1e-12)
    assert res["count"].tolist() == [5, 0]
    vf = res["valid_fraction"]
    assert vf.shape == (2, 3, 2) and np.isnan(vf[1]).all()
    assert np.allclose(vf[0, 1:], 1.0, rtol=1e-14) and 0.97 < vf[0, 0, 1] < 1.0 - 1e-6
    assert abs(vf[0, 0, 0] - 1.0) < 1e-14                                # the NaN cell's row lies outside "nh"
    assert res["labels"] == ["rain", "gale", "cold"] and res["bands"] == ["nh", "all"]
    assert res["directions"] == ["ge", "ge", "le"] and res["thresholds"][1] == [float(np.float32(17.2))]
    e.reset()
    assert int(e.acc.abs().sum()) == 0 and int(e.n_samples.sum()) == 0


def test_event_table_sync_dist_makes_one_all_reduce(tmp_path, monkeypatch):
    import torch.distributed as dist
    e, _ = _filled()
    want = e.counts()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        calls = []
        real = dist.all_reduce
        monkeypatch.setattr(dist, "all_reduce", lambda t, **kw: (calls.append((tuple(t.shape), t.dtype)), real(t, **kw))[1])
        got = e.counts(sync_dist=True)
        assert calls == [((e.acc.numel() + 2,), torch.int64)]
    finally:
        dist.destroy_process_group()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_event_table_prints():
    e, _ = _filled()
    res = e.result()
    text = EV.EventTable.table(res, "rain")
    lines = text.split("\n")
    assert lines[0] == "rain / nh"
    blocks = "\n".join(lines[1:]).split("\n\n")
    assert [b.split()[0] for b in blocks] == ["frequency_bias", "csi", "ets", "sedi"]
    assert lines[1].split() == ["frequency_bias", "count", ">=1", ">=5", ">=0.2"]
    assert lines[2].split()[:2] == ["0", "5"] and lines[3].split() == ["1", "0", "nan", "nan", "nan"]
    assert float(lines[2].split()[2]) == pytest.approx(res["frequency_bias"][0, 0, 0, 0], abs=5e-5)
    assert len({len(line) for line in blocks[0].split("\n")}) == 1               # aligned columns
    cold = EV.EventTable.table(res, "cold", band="all", metrics=("hits", "pod"))
    assert cold.split("\n")[0] == "cold / all" and cold.split("\n")[1].split() == ["hits", "count", "<=-5", "<=-10"]
    for kw, word in ((dict(label="fog"), "fog"), (dict(label="rain", band="sh"), "sh"),
                     (dict(label="rain", metrics=("rmse",)), "rmse")):
        with pytest.raises(ValueError, match=word):
            EV.EventTable.table(res, **kw)


# ================================================================================================ 4. the forecaster hook
def test_forecaster_run_refusals_with_events():
    from paradis_model_amd.forecast import Forecaster, PostSpec
    H, W = 5, 8
    names = NAMES[:3]
    ev = {"rain": {"source": "tp", "thresholds": [1.0]}}
    spec = PostSpec.from_features(names, [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    fc = Forecaster(None, spec, LAT, np.zeros(W), graph=False)
    inp, forc, const = torch.zeros(1, 1, 6, H, W), torch.zeros(1, 2, H, W, 1), torch.zeros(1, 1, H, W, 1)
    table = lambda n=2, nm=names: EV.EventTable(nm, LAT, n, ev, device="cpu")     # noqa: E731
    with pytest.raises(ValueError, match="event table needs truth"):
        fc.run(inp, forc, const, None, events=table(), truth=None)
    good = torch.zeros(1, 2, 3, H, W)
    args = (None, good, False, None, 1, 2, 3, H, W, None)
    with pytest.raises(ValueError, match="truth"):
        fc._check_verification(None, good[:, :1], False, None, 1, 2, 3, H, W, None, table())
    with pytest.raises(ValueError, match="event table has 1 leads"):
        fc._check_verification(*args, table(1))
    with pytest.raises(ValueError, match="event table's names"):
        fc._check_verification(*args, table(2, ["tp", "v10", "u10"]))
    with pytest.raises(ValueError, match="clim_index must be int32"):
        fc._check_verification(None, good, False, torch.zeros(1, 2), 1, 2, 3, H, W, None, table())
    with pytest.raises(ValueError, match="scorecard"):                  # as before: truth alone goes with nothing
        fc._check_verification(None, good, False, None, 1, 2, 3, H, W)
    with pytest.raises(RuntimeError, match="MI355X"):                   # every host check passed: the device check
        fc._check_verification(*args, table())


# ================================================================================================ 5. the C ABI
def test_events_symbols_are_declared_exported_and_bound():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS + ("paradis_events_max_sources",):
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    sig = _lib.SIGNATURES["paradis_events_update"][1]
    assert len(sig) == 18 and sig[1] is ctypes.c_int64 and sig[3] is ctypes.c_int64 and sig[6] is ctypes.c_int
    assert _lib.SIGNATURES["paradis_events_ws_bytes"][0] is ctypes.c_size_t
    L = _lib.lib
    assert L.paradis_abi_version() == 10
    assert L.paradis_events_max_thresholds() == 8 and L.paradis_events_max_sources() >= 6
    piece = L.paradis_verify_piece()
    assert L.paradis_events_rows(64) == piece // 64 == 128 and L.paradis_events_rows(1440) == 5
    assert L.paradis_events_rows(piece) == 1 and L.paradis_events_rows(10 * piece) == 1 and L.paradis_events_rows(1) == piece
    assert L.paradis_events_rows(0) == 0
    with open(os.path.join(ROOT, "paradis_model_amd", "csrc", "Makefile")) as f:
        assert "FLAGS_events := -ffp-contract=off" in f.read()


def test_events_workspace_holds_the_partials():
    """uint32 [B][S][H][1 + 3 TMAX]; 0 for empty shapes"""
    from paradis_model_amd import _lib
    L = _lib.lib
    for (B, S, H, W) in ((2, 3, 32, 64), (1, 6, 721, 1440), (5, 1, 1, 64)):
        assert L.paradis_events_ws_bytes(B, S, H, W) == B * S * H * 25 * 4
    for shape in ((0, 3, 32, 64), (2, 0, 32, 64), (2, 3, 0, 64), (2, 3, 32, 0), (-1, 3, 32, 64)):
        assert L.paradis_events_ws_bytes(*shape) == 0


def test_events_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first
    TM = L.paradis_events_max_thresholds()

    def call(word, fc=fake, truth=fake, clim=None, idx=None, K=0, src=((0, 0, 0, 1),), sign=1.0, acc=fake, n=fake,
             ws=fake, B=2, C=3, S=None, H=4, W=8, fc_bs=96, truth_bs=96):
        st = np.ascontiguousarray(np.array(src, np.int32).reshape(-1, 4))
        tt = np.zeros((len(st), 1 + TM), np.float32)
        tt[:, 0] = sign
        S = len(st) if S is None else S
        rc = L.paradis_events_update(fc, fc_bs, truth, truth_bs, clim, idx, K, st.ctypes.data, tt.ctypes.data, acc, n,
                                     ws, B, C, S, H, W, None)
        assert rc == 1 and word in _lib.last_error(), (word, rc, _lib.last_error())

    call("bad shape", B=-1)
    call("bad shape", C=0)
    call("bad shape", H=0)
    call("bad shape", W=0)
    call("bad shape", S=0)
    call("bad shape", src=((0, 0, 0, 1),) * (L.paradis_events_max_sources() + 1))
    call("go together", clim=fake)
    call("go together", idx=fake)
    call("K must be", clim=fake, idx=fake, K=0)
    call("too large", H=1 << 16, W=1 << 15, fc_bs=1 << 40, truth_bs=1 << 40)
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
    call("missing", ws=None)
    call("null input", fc=None)
    # B == 0 does nothing and asks for nothing
    st, tt = np.zeros((1, 4), np.int32), np.zeros((1, 1 + TM), np.float32)
    assert L.paradis_events_update(None, 0, None, 0, None, None, 0, st.ctypes.data, tt.ctypes.data, None, None, None, 0, 3,
                                   1, 4, 8, None) == 0
