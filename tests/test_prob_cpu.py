"""Host side of the probabilistic event verification, no GPU: the numpy oracle's own closed forms (tests/prob_oracle.py),
the argument checks and host arithmetic of ``probability.ProbabilityTable`` on ``device="cpu"``, the
``Forecaster.run(probability=...)`` refusals and the C ABI's refusals before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from paradis_model_amd import probability as PR
from tests import prob_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tp", "u10", "v10", "t2m"]
LAT = np.linspace(-80.0, 80.0, 5)
SYMBOLS = ("paradis_prob_max_members", "paradis_prob_rows", "paradis_prob_counters", "paradis_prob_ws_bytes",
           "paradis_prob_update")
F32 = np.float32
EVENTS = {"wet": {"source": "tp", "thresholds": [0.5, 1.0, 0.0]},
          "wind": {"source": ("speed", "u10", "v10"), "thresholds": [1.0]},
          "cold": {"source": ("anomaly", "t2m"), "thresholds": [-0.5, 0.25], "direction": "le"}}
SOURCES = [{"kind": "plain", "c0": 0, "thresholds": [0.5, 1.0, 0.0], "direction": "ge"},
           {"kind": "speed", "c0": 1, "c1": 2, "thresholds": [1.0], "direction": "ge"},
           {"kind": "anomaly", "c0": 3, "thresholds": [-0.5, 0.25], "direction": "le"}]


def counts_of(p_members, o, M):
    """``(N0[k], N1[k])`` of per-cell member counts ``p_members`` (0 .. M) and outcomes ``o``"""
    k, o = np.asarray(p_members).reshape(-1), np.asarray(o).reshape(-1).astype(bool)
    return np.bincount(k[~o], minlength=M + 1), np.bincount(k[o], minlength=M + 1)


# ================================================================================================ 1. the oracle itself
def test_oracle_perfectly_reliable_counts_have_no_reliability_term():
    """N_1k / N_k = k / M in every bin: reliability == 0 and brier == uncertainty - resolution"""
    M = 4
    Nk = np.array([40, 80, 120, 80, 40])
    N1 = Nk * np.arange(M + 1) // M
    s = PO.scores_of(Nk - N1, N1, M)
    assert s["reliability"] == 0.0
    assert abs(s["brier"] - (s["uncertainty"] - s["resolution"])) <= 1e-15
    assert s["observed_frequency"] == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert s["base_rate"] == 0.5 and abs(sum(s["forecast_frequency"]) - 1.0) <= 1e-15


def test_oracle_decomposition_identity():
    rng = np.random.default_rng(1)
    for M in (2, 3, 5, 16, 32):
        for _ in range(20):
            N0 = rng.integers(0, 50, M + 1) * rng.integers(0, 2, M + 1)          # some empty bins
            N1 = rng.integers(0, 50, M + 1) * rng.integers(0, 2, M + 1)
            if N0.sum() == 0 or N1.sum() == 0:
                continue
            w = rng.random()                                                   # weighted counts, as after the bands
            s = PO.scores_of(w * N0, w * N1, M)
            assert abs(s["brier"] - (s["reliability"] - s["resolution"] + s["uncertainty"])) <= 1e-12, M
            assert 0.0 <= s["roc_area"] <= 1.0 and s["pod"][0] == 1.0 and s["pofd"][0] == 1.0
            assert abs(s["bss"] - (s["resolution"] - s["reliability"]) / s["uncertainty"]) <= 1e-10


def test_oracle_roc_area_is_the_mann_whitney_statistic():
    rng = np.random.default_rng(2)
    for M in (2, 5, 16):
        n = 600
        o = rng.random(n) < 0.3
        k = np.clip(np.round(M * (0.3 + 0.35 * o + 0.25 * rng.standard_normal(n))), 0, M).astype(np.int64)
        N0, N1 = counts_of(k, o, M)
        s = PO.scores_of(N0, N1, M)
        want = PO.mann_whitney(k / M, o)
        assert abs(s["roc_area"] - want) <= 1e-12, (M, s["roc_area"], want)
        assert want > 0.6
    assert PO.mann_whitney([0.5, 0.5], [1, 0]) == 0.5 and PO.mann_whitney([1.0, 0.0], [1, 0]) == 1.0


def test_oracle_fair_brier_is_unbiased_in_the_member_count():
    """a calibrated synthetic ensemble - per cell a probability p, the truth and every member Bernoulli(p) -: the fair
    Brier score at M = 2 and at M = 16 agree within sampling error (both estimate E p (1 - p)); the ensemble's own Brier
    score carries E p (1 - p) / M on top and does not"""
    rng = np.random.default_rng(3)
    n = 200_000
    p = rng.random(n)
    o = rng.random(n) < p
    out = {}
    for M in (2, 16):
        k = (rng.random((M, n)) < p[None]).sum(axis=0)
        out[M] = PO.scores_of(*counts_of(k, o, M), M)
    expect = 1.0 / 6.0                                                         # E p (1 - p), p uniform
    sigma = 0.5 / np.sqrt(n)                                                   # a per-cell term lies in [0, 1]
    for M in (2, 16):
        assert abs(out[M]["brier_fair"] - expect) <= 5 * sigma, (M, out[M]["brier_fair"])
        assert abs(out[M]["brier"] - expect * (1.0 + 1.0 / M)) <= 5 * sigma, (M, out[M]["brier"])
    assert abs(out[2]["brier_fair"] - out[16]["brier_fair"]) <= 10 * sigma
    assert out[2]["brier"] - out[16]["brier"] > 40 * sigma


def test_oracle_two_members_closed_form():
    """M = 2: the Brier score of p = k / 2 by hand, and Ferro's correction k (M - k) / (M^2 (M - 1)) = 1/4 at k = 1"""
    N0, N1 = [5.0, 3.0, 1.0], [2.0, 4.0, 6.0]
    s = PO.scores_of(N0, N1, 2)
    n = 21.0
    brier = (2 * 1.0 + 4 * 0.25 + 3 * 0.25 + 1 * 1.0) / n
    assert abs(s["brier"] - brier) <= 1e-15 and abs(s["brier_fair"] - (brier - 7 * 0.25 / n)) <= 1e-15
    assert s["pod"] == [1.0, 10.0 / 12.0, 0.5] and s["pofd"] == [1.0, 4.0 / 9.0, 1.0 / 9.0]
    area = (1 - 4 / 9) * (1 + 10 / 12) / 2 + (4 / 9 - 1 / 9) * (10 / 12 + 0.5) / 2 + (1 / 9) * 0.5 / 2
    assert abs(s["roc_area"] - area) <= 1e-15


def test_oracle_zero_denominators_give_nan():
    s = PO.scores_of([3.0, 0.0, 1.0], [0.0, 0.0, 0.0], 2)                     # no truth event at all
    assert s["base_rate"] == 0.0 and s["uncertainty"] == 0.0 and np.isnan(s["bss"]) and np.isnan(s["roc_area"])
    assert np.isnan(s["observed_frequency"][1]) and s["observed_frequency"][0] == 0.0 and np.isnan(s["pod"][0])
    s = PO.scores_of([0.0] * 3, [0.0] * 3, 2)
    assert all(np.isnan(s[k]) for k in PO.SCORES)


def _states(seed, G, M, C=4, H=5, W=8):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((G, C, H, W)).astype(F32)
    f = (np.repeat(t, M, axis=0) + rng.standard_normal((G * M, C, H, W)) * 0.7).astype(F32)
    clim = (rng.standard_normal((2, C, H, W)) * 0.3).astype(F32)
    return f, t, clim


def test_oracle_joint_rows_invariants_and_invalid_cells():
    M, G = 3, 2
    f, t, clim = _states(5, G, M)
    f[1, 0, 2, 3] = np.nan                     # member 1 of ensemble 0, channel tp
    t[1, 1, 0, 0] = np.inf                     # truth of ensemble 1, channel u10: the speed source
    clim[1, 3, 4, 7] = np.nan                  # slot 1, t2m: ensemble 1's anomaly
    acc, detail = PO.joint_rows(f, t, M, SOURCES, clim, [0, 1])
    nV, joint = PO.split(acc, M)
    assert acc.shape == (3, 5, 1 + 3 * 2 * 4) and joint.shape == (3, 5, 3, 2, 4)
    assert nV[0].tolist() == [16, 16, 15, 16, 16] and nV[1].tolist() == [15, 16, 16, 16, 16]
    assert nV[2].tolist() == [16, 16, 16, 16, 15]
    for s, src in enumerate(SOURCES):
        nt = len(src["thresholds"])
        assert (joint[s, :, :nt].sum(axis=(-1, -2)) == nV[s][:, None]).all()
        assert (joint[s, :, nt:] == 0).all()
    # an ensemble whose slot is out of range: nothing for the anomaly source, everything for the others
    acc2, _ = PO.joint_rows(f, t, M, SOURCES, clim, [0, 2])
    acc1, _ = PO.joint_rows(f[:M], t[:1], M, SOURCES, clim, [0])
    assert np.array_equal(acc2[2], acc1[2]) and np.array_equal(acc2[:2], acc[:2])
    # the speed is mul, mul, add, sqrt in float32; the "le" event is sign = -1
    x, _ = PO.source_value(t, "speed", 1, 2, None)
    assert x.dtype == F32 and np.array_equal(x[0], np.sqrt(t[0, 1] * t[0, 1] + t[0, 2] * t[0, 2]))
    valid, o, k, xt = detail[2]
    assert np.array_equal(o[1][valid], (xt <= F32(0.25))[valid])


# ================================================================================================ 2. ProbabilityTable on the host
def _table(**kw):
    kw.setdefault("bands", {"nh": (20, 90), "global": (-90, 90)})
    kw.setdefault("members", 3)
    kw.setdefault("events", EVENTS)
    kw.setdefault("climatology", torch.zeros(2, 4, 5, 8))
    return PR.ProbabilityTable(NAMES, LAT, 2, device="cpu", **kw)


def test_table_shapes_and_memory():
    e = _table()
    assert PR.max_members() == 32
    assert e.T == 3 and e.members == 3 and e.labels == ["wet", "wind", "cold"] and e.n_thresholds == [3, 1, 2]
    assert e.acc.shape == (2, 3, 5, 1 + 3 * 2 * 4) and e.acc.dtype == torch.int64 and e.n_samples.dtype == torch.int64
    assert e.kinds == [0, 1, 2] and e._bytes_per_cell == 4 * 4 + 8 * 4 + 4 * 4 + 4 and e.TAKES_CLIM_INDEX
    assert e.band_w.shape == (2, 5) and e.band_w[0, :3].tolist() == [0.0, 0.0, 0.0]
    assert e._thr[2, :3].tolist() == [-1.0, 0.5, -0.25]
    assert (e.NOUN, e.HAS, e.NEEDS) == ("the probability table", "the probability table has",
                                       "a probability table needs")
    # 190 MB at 40 leads, 6 sources, 721 rows, T = 4, M = 16
    assert 8 * 40 * 6 * 721 * (1 + 4 * 2 * 17) == 189_651_840
    assert [PR.bytes_per_cell(k, 16) for k in (0, 1, 2)] == [68, 136, 72]


def test_table_constructor_errors():
    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            _table(**kw)

    for m in (1, 0, PR.max_members() + 1, 2.5, True):
        bad("ProbabilityTable: members must be", members=m)
    bad("events must be a non-empty dict", events={})
    bad("not among the names", events={"x": {"source": "q700", "thresholds": [1.0]}})
    bad("9 thresholds", events={"x": {"source": "tp", "thresholds": list(range(9))}})
    bad("direction", events={"x": {"source": "tp", "thresholds": [1.0], "direction": "gt"}})
    bad("finite", events={"x": {"source": "tp", "thresholds": [np.nan]}})
    bad("with itself", events={"x": {"source": ("speed", "tp", "tp"), "thresholds": [1.0]}})
    bad("is an anomaly, but the table has no climatology", climatology=None)
    bad("climatology must be", climatology=torch.zeros(2, 3, 5, 8))
    bad("ProbabilityTable: band 'x'", bands={"x": (10, -10)})
    bad("bands must be", bands={})
    bad("weights", weights=torch.ones(4))
    many = {f"e{i}": {"source": "tp", "thresholds": [float(i)]} for i in range(17)}
    bad("at most 16", events=many)
    for n_leads in (0, 1.5, True):
        with pytest.raises(ValueError, match="n_leads"):
            PR.ProbabilityTable(NAMES, LAT, n_leads, {"x": {"source": "tp", "thresholds": [1.0]}}, 4, device="cpu")
    with pytest.raises(ValueError, match="lat_deg"):
        PR.ProbabilityTable(NAMES, [0.0, 91.0], 1, {"x": {"source": "tp", "thresholds": [1.0]}}, 4, device="cpu")
    with pytest.raises(ValueError, match="names must list"):
        PR.ProbabilityTable([], LAT, 1, {"x": {"source": "tp", "thresholds": [1.0]}}, 4, device="cpu")


def test_table_update_argument_errors_on_cpu_tensors():
    e = _table()
    f, t = torch.zeros(6, 4, 5, 8), torch.zeros(2, 4, 5, 8)
    idx = torch.zeros(2, dtype=torch.int32)

    def bad(match, lead=0, fc=f, truth=t, k=idx, exc=ValueError, table=e):
        with pytest.raises(exc, match=match):
            table.update(lead, fc, truth, k)

    bad("lead", lead=2)
    bad("lead", lead=True)
    bad("float32", fc=f.double())
    bad("float32", truth=t.double())
    bad(r"\[B, C, H, W\]", truth=t[0])
    bad("the table has 4 channels and 5 latitudes", fc=torch.zeros(6, 3, 5, 8))
    bad("5 states are not whole ensembles of 3 members", fc=f[:5])
    bad("2 ensembles of 3 members need truth", truth=torch.zeros(6, 4, 5, 8))
    bad("truth is", truth=torch.zeros(2, 4, 5, 6))
    bad("forecast must hold dense", fc=torch.zeros(6, 4, 5, 16)[..., ::2])
    bad("truth must hold dense", truth=torch.zeros(2, 4, 5, 16)[..., ::2])
    bad("clim_index is needed to choose among the 2", k=None)
    bad(r"clim_index must be an int32 tensor \[2\]", k=torch.zeros(6, dtype=torch.int32))      # one slot per ENSEMBLE
    bad(r"clim_index must be an int32 tensor \[2\]", k=torch.zeros(2, dtype=torch.int64))
    bad("forecast has 6 longitudes, the climatology 8", fc=torch.zeros(6, 4, 5, 6), truth=torch.zeros(2, 4, 5, 6))
    plain = _table(events={"wet": EVENTS["wet"]}, climatology=None)
    bad("clim_index given, but the table has no climatology", table=plain)
    plain.bind(8)
    bad("forecast has 6 longitudes, the table is bound to 8", fc=torch.zeros(6, 4, 5, 6), truth=torch.zeros(2, 4, 5, 6),
        k=None, table=plain)
    with pytest.raises(ValueError, match="bound to 8 longitudes already"):
        plain.bind(6)
    with pytest.raises(ValueError, match="W must be an integer >= 1"):
        plain.bind(0)
    bad("MI355X", exc=RuntimeError)                                      # every host check passed: the device check
    bad("MI355X", fc=torch.zeros(6, 3, 4, 5, 8)[:, 1], truth=torch.zeros(6, 4, 5, 8)[::3], exc=RuntimeError)
    assert int(e.acc.abs().sum()) == 0


def _filled():
    """a table whose accumulators are filled by hand with the oracle's rows of two updates at lead 0"""
    M = 3
    e = _table(members=M)
    e.bind(8)
    acc = 0
    for seed, G, idx in ((7, 2, [0, 1]), (8, 1, [1])):
        f, t, clim = _states(seed, G, M)
        f[0, 2, 2, 1] = np.nan
        a, _ = PO.joint_rows(f, t, M, SOURCES, clim, idx)
        acc = acc + a
    e.acc[0] = torch.from_numpy(acc)
    e.n_samples[0] = 3
    return e, acc


def test_table_result_from_hand_filled_accumulators():
    e, acc = _filled()
    M = 3
    cnt = e.counts()
    nV, joint = PO.split(acc, M)
    assert cnt["valid"].dtype == np.int64 and cnt["joint"].dtype == np.int64 and cnt["n_samples"].tolist() == [3, 0]
    assert np.array_equal(cnt["valid"][0], nV) and cnt["joint"].shape == (2, 3, 5, 3, 2, 4)
    for s, nt in enumerate(e.n_thresholds):
        assert np.array_equal(cnt["joint"][0, s, :, :nt], joint[s, :, :nt])
        assert (cnt["joint"][:, s, :, nt:] == -1).all()
    assert cnt["valid"][0, 1, 2] == 3 * 8 - 2                            # the NaN member cell of v10, in both updates
    res = e.result()
    want = PO.report(acc, e.band_w, M, e.n_thresholds)
    for k in PR.SCORES + PR.CURVES:
        got = res[k]
        assert got.dtype == np.float64 and got.shape[:4] == (2, 3, 2, 3), k
        assert np.isnan(got[1]).all(), k                                 # lead 1 was never updated
        assert np.array_equal(np.isnan(got[0]), np.isnan(want[k])), k
        err = np.abs(got[0] - want[k])[~np.isnan(want[k])]
        assert err.max() <= 1e-12, (k, float(err.max()))
    for s, nt in enumerate(e.n_thresholds):                             # NaN past a source's own thresholds
        assert np.isnan(res["brier"][0, s, :, nt:]).all() and np.isfinite(res["brier"][0, s, :, :nt]).all()
    live = np.isfinite(res["brier"][0])
    ident = res["reliability"][0] - res["resolution"][0] + res["uncertainty"][0]
    assert np.abs(res["brier"][0] - ident)[live].max() <= 1e-12
    assert (res["brier_fair"][0][live] <= res["brier"][0][live]).all()
    assert res["pod"].shape == (2, 3, 2, 3, 4) and (res["pod"][0, ..., 0][live] == 1.0).all()
    assert np.abs(np.nansum(res["forecast_frequency"][0], axis=-1)[live] - 1.0).max() <= 1e-12
    seen = 3 * 8 * e.band_w.sum(axis=1)
    assert np.abs(res["valid_fraction"][0] - want["valid"] / seen[None, :]).max() <= 1e-15
    assert (res["valid_fraction"][0] <= 1.0).all() and np.isnan(res["valid_fraction"][1]).all()
    assert res["count"].tolist() == [3, 0] and res["labels"] == ["wet", "wind", "cold"] and res["members"] == 3
    assert res["bands"] == ["nh", "global"] and res["directions"] == ["ge", "ge", "le"]
    assert res["thresholds"] == [[0.5, 1.0, 0.0], [1.0], [-0.5, 0.25]]
    e.reset()
    assert int(e.acc.abs().sum()) == 0 and int(e.n_samples.sum()) == 0
    assert all(np.isnan(e.result()[k]).all() for k in PR.SCORES + PR.CURVES)


def test_table_nan_rules():
    """a zero denominator gives NaN: no truth event (bss, roc_area, pod), an empty forecast bin (observed_frequency),
    a band without a valid cell (everything)"""
    M = 2
    e = PR.ProbabilityTable(["tp"], LAT, 1, {"wet": {"source": "tp", "thresholds": [1.0, 2.0]}}, M, device="cpu",
                            bands={"sh": (-90, -20), "nh": (20, 90)})
    e.bind(8)
    acc = np.zeros((1, 5, 1 + 2 * 2 * 3), np.int64)
    acc[0, 3:, 0] = 8                                                     # rows of the northern band only
    acc[0, 3:, 1 + 0] = 5                                                 # threshold 0: o = 0, k = 0 ..
    acc[0, 3:, 1 + 2] = 3                                                 # .. and o = 0, k = 2: no truth event
    acc[0, 3:, 1 + 6 + 0] = 4                                             # threshold 1: o = 0, k = 0
    acc[0, 3:, 1 + 6 + 3 + 2] = 4                                         # and o = 1, k = 2: a perfect forecast
    e.acc[0] = torch.from_numpy(acc)
    e.n_samples[0] = 1
    r = e.result()
    assert all(np.isnan(r[k][0, 0, 0]).all() for k in PR.SCORES + PR.CURVES)          # the southern band: N = 0
    assert r["valid_fraction"][0, 0, 0] == 0.0 and abs(r["valid_fraction"][0, 0, 1] - 1.0) <= 1e-15
    nh = {k: r[k][0, 0, 1] for k in PR.SCORES + PR.CURVES}
    assert nh["base_rate"][0] == 0.0 and nh["uncertainty"][0] == 0.0 and np.isnan(nh["bss"][0])
    assert np.isnan(nh["roc_area"][0]) and np.isnan(nh["pod"][0]).all()
    assert np.abs(nh["pofd"][0] - [1.0, 0.375, 0.375]).max() <= 1e-15
    assert np.isnan(nh["observed_frequency"][0, 1]) and nh["observed_frequency"][0, 0] == 0.0
    assert abs(nh["brier"][0] - 3.0 / 8.0) <= 1e-15 and nh["brier_fair"][0] == nh["brier"][0]
    assert nh["brier"][1] == 0.0 and nh["reliability"][1] == 0.0 and nh["resolution"][1] == 0.25
    assert nh["bss"][1] == 1.0 and nh["roc_area"][1] == 1.0 and nh["base_rate"][1] == 0.5


def test_table_sync_dist_makes_one_all_reduce(tmp_path, monkeypatch):
    import torch.distributed as dist
    e, _ = _filled()
    want = e.result()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        calls = []
        real = dist.all_reduce
        monkeypatch.setattr(dist, "all_reduce", lambda t, **kw: (calls.append((tuple(t.shape), t.dtype)), real(t, **kw))[1])
        got = e.result(sync_dist=True)
        assert calls == [((e.acc.numel() + 2,), torch.int64)]
    finally:
        dist.destroy_process_group()
    for k in PR.SCORES + PR.CURVES + ("count", "valid_fraction"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_table_prints():
    e, _ = _filled()
    res = e.result()
    text = PR.ProbabilityTable.table(res, "wet", band="global", threshold=1)
    lines = text.split("\n")
    assert lines[0] == "wet >= 1 / global / 3 members"
    assert lines[1].split() == ["lead", "count"] + list(PR.SCORES)
    assert lines[2].split()[:2] == ["0", "3"] and lines[3].split() == ["1", "0"] + ["nan"] * 8
    assert float(lines[2].split()[2]) == pytest.approx(res["brier"][0, 0, 1, 1], rel=1e-4)
    assert lines[4] == "" and lines[5].split() == ["lead", "p", "=", "k", "/", "M", "0.000", "0.333", "0.667", "1.000"]
    assert lines[6].split()[:2] == ["0", "forecast"] and lines[7].split()[:2] == ["0", "observed"]
    assert sum(float(v) for v in lines[6].split()[2:]) == pytest.approx(1.0, abs=1e-3)
    assert lines[9].split() == ["1", "observed"] + ["nan"] * 4 and len(lines) == 10
    assert len({len(ln) for ln in lines[1:4]}) == 1 and len({len(ln) for ln in lines[5:]}) == 1     # aligned columns
    assert PR.ProbabilityTable.table(res, "cold").split("\n")[0] == "cold <= -0.5 / nh / 3 members"
    for kw, word in ((dict(label="dry"), "dry"), (dict(label="wet", band="sh"), "sh"),
                     (dict(label="wind", threshold=1), "threshold"), (dict(label="wet", threshold=True), "threshold")):
        with pytest.raises(ValueError, match=word):
            PR.ProbabilityTable.table(res, **kw)


# ================================================================================================ 3. the forecaster hook
def test_forecaster_run_refusals_with_a_probability_table():
    from paradis_model_amd.ensemble import EnsembleCard
    from paradis_model_amd.forecast import Forecaster, PostSpec
    from paradis_model_amd.verify import Scorecard
    H, W = 5, 8
    names = NAMES[:3]
    spec = PostSpec.from_features(names, [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    fc = Forecaster(None, spec, LAT, np.zeros(W), graph=False)
    inp, forc, const = torch.zeros(4, 1, 6, H, W), torch.zeros(4, 2, H, W, 1), torch.zeros(4, 1, H, W, 1)
    ev = {"wet": {"source": "tp", "thresholds": [1.0]}}
    table = lambda n=2, nm=names, m=2: PR.ProbabilityTable(nm, LAT, n, ev, m, device="cpu")     # noqa: E731
    with pytest.raises(ValueError) as e:
        fc.run(inp, forc, const, None, probability=table(), truth=None)
    assert str(e.value) == "Forecaster.run: a probability table needs truth [B, n_stored, C, H, W] on the device"
    good = torch.zeros(4, 2, 3, H, W)
    kw = dict(scorecard=None, truth=good, truth_normalized=False, clim_index=None, B=4, n_stored=2, C=3, H=H, W=W)
    with pytest.raises(ValueError, match="truth must be float32"):
        fc._check_verification(**{**kw, "truth": good[:, :1]}, probability=table())
    with pytest.raises(ValueError) as e:
        fc._check_verification(**kw, probability=table(1))
    assert str(e.value) == "Forecaster.run: the probability table has 1 leads, the rollout stores 2"
    with pytest.raises(ValueError) as e:
        fc._check_verification(**kw, probability=table(2, ["tp", "v10", "u10"]))
    assert str(e.value) == \
        "Forecaster.run: the probability table's names are not the chunk's channel names (PostSpec.names)"
    with pytest.raises(ValueError) as e:
        fc._check_verification(**kw, probability=table(m=3))
    assert str(e.value) == \
        "Forecaster.run: the probability table has 3 members, a batch of 4 states is not whole ensembles"
    with pytest.raises(ValueError, match=r"clim_index must be int32 \(4, 2\)"):       # the table takes a clim_index
        fc._check_verification(**{**kw, "clim_index": torch.zeros(4, 3, dtype=torch.int32)}, probability=table())
    # the scorecard speaks first, the ensemble card before the probability table
    with pytest.raises(ValueError, match="the scorecard has 1 leads"):
        fc._check_verification(**{**kw, "scorecard": Scorecard(names, np.ones(H), 1, device="cpu")},
                               probability=table(1))
    with pytest.raises(ValueError, match="the ensemble card has 3 members"):
        fc._check_verification(**kw, ensemble=EnsembleCard(names, LAT, 2, 3, device="cpu"), probability=table(m=3))
    with pytest.raises(RuntimeError, match="MI355X"):                   # every host check passed: the device check
        fc._check_verification(**kw, probability=table())
    with pytest.raises(ValueError, match="scorecard"):                  # as before: truth alone goes with nothing
        fc._check_verification(**kw)


# ================================================================================================ 4. the C ABI
def test_prob_symbols_are_declared_exported_and_bound():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    sig = _lib.SIGNATURES["paradis_prob_update"][1]
    assert len(sig) == 20 and sig[1] is ctypes.c_int64 and sig[3] is ctypes.c_int64 and sig[6] is ctypes.c_int
    assert _lib.SIGNATURES["paradis_prob_ws_bytes"][0] is ctypes.c_size_t
    L = _lib.lib
    assert L.paradis_abi_version() == 10
    assert L.paradis_prob_max_members() == 32 == L.paradis_ens_max_members()
    for W in (1, 3, 4, 64, 66, 260, 1440, 100000):
        assert L.paradis_prob_rows(W) >= 4 and L.paradis_prob_rows(W) % 4 == 0, W    # equal work for the four waves
    assert [L.paradis_prob_rows(W) for W in (1, 64, 66, 260, 1440)] == [1024, 16, 12, 4, 4]
    assert L.paradis_prob_rows(0) == 0 and L.paradis_prob_rows(-3) == 0
    with open(os.path.join(ROOT, "paradis_model_amd", "csrc", "Makefile")) as f:
        assert "FLAGS_probability := -ffp-contract=off" in f.read()


def test_prob_counters_and_workspace():
    """uint32 [G][S][H][1 + 2 T (M + 1)]; 0 for empty shapes and for an M or T outside its range"""
    from paradis_model_amd import _lib
    L = _lib.lib
    tmax = L.paradis_events_max_thresholds()
    for (M, T) in ((2, 1), (16, 4), (32, 8), (5, 3)):
        assert L.paradis_prob_counters(M, T) == 1 + 2 * T * (M + 1)
    assert L.paradis_prob_counters(32, tmax) == 529
    for (M, T) in ((1, 1), (33, 1), (4, 0), (4, tmax + 1), (0, 0), (-1, 2)):
        assert L.paradis_prob_counters(M, T) == 0
    for (G, S, H, W, M, T) in ((2, 3, 32, 64, 4, 2), (1, 6, 721, 1440, 16, 4), (5, 1, 1, 64, 2, 1), (3, 16, 9, 260, 32, 8)):
        assert L.paradis_prob_ws_bytes(G, S, H, W, M, T) == G * S * H * (1 + 2 * T * (M + 1)) * 4
    for shape in ((0, 3, 32, 64, 4, 2), (2, 0, 32, 64, 4, 2), (2, 3, 0, 64, 4, 2), (2, 3, 32, 0, 4, 2),
                  (2, 3, 32, 64, 1, 2), (2, 3, 32, 64, 33, 2), (2, 3, 32, 64, 4, 0), (2, 3, 32, 64, 4, tmax + 1),
                  (-1, 3, 32, 64, 4, 2)):
        assert L.paradis_prob_ws_bytes(*shape) == 0


def test_prob_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    tmax = L.paradis_events_max_thresholds()
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first
    src_ok = np.array([[0, 0, 0, 2], [1, 1, 2, 1]], np.int32)
    thr_ok = np.zeros((2, 1 + tmax), np.float32)
    thr_ok[:, 0] = 1.0

    def call(word, fc=fake, truth=fake, clim=None, idx=None, K=0, src=src_ok, thr=thr_ok, acc=fake, n=fake, ws=fake, G=2,
             M=4, T=2, C=3, S=2, H=4, W=8, fc_bs=96, truth_bs=96):
        sp = None if src is None else src.ctypes.data_as(ctypes.c_void_p)
        tp = None if thr is None else thr.ctypes.data_as(ctypes.c_void_p)
        rc = L.paradis_prob_update(fc, fc_bs, truth, truth_bs, clim, idx, K, sp, tp, acc, n, ws, G, M, T, C, S, H, W,
                                   None)
        assert rc == 1 and word in _lib.last_error(), (word, rc, _lib.last_error())

    def src_with(row, s=0):
        t = src_ok.copy()
        t[s] = row
        return t

    call("bad shape", G=-1)
    call("bad shape", C=0)
    call("bad shape", S=0)
    call("bad shape", S=L.paradis_events_max_sources() + 1)
    call("bad shape", H=0)
    call("bad shape", W=0)
    call("go together", clim=fake)
    call("go together", idx=fake)
    call("must be >= 1", clim=fake, idx=fake, K=0)
    call("members", M=1)
    call("members", M=0)
    call("members", M=L.paradis_prob_max_members() + 1)
    call("thresholds per source", T=0)
    call("thresholds per source", T=tmax + 1)
    call("missing", acc=None)
    call("missing", n=None)
    call("missing", ws=None)
    call("null input", fc=None)
    call("null input", truth=None)
    call("null input", src=None)
    call("null input", thr=None)
    call("strides", fc_bs=95)
    call("strides", truth_bs=95)
    call("too large", H=1 << 16, W=1 << 15, fc_bs=1 << 40, truth_bs=1 << 40)
    call("has kind", src=src_with((3, 0, 0, 1)))
    call("no climatology", src=src_with((2, 0, 0, 1)))
    call("outside [0, 3)", src=src_with((0, 3, 0, 1)))
    call("outside [0, 3)", src=src_with((1, 1, 3, 1), s=1))
    call("thresholds, outside", src=src_with((0, 0, 0, 0)))
    call("thresholds, outside", src=src_with((0, 0, 0, tmax + 1)))
    call("the accumulator row holds T = 1", T=1)                          # source 0 has two thresholds
    bad_sign = thr_ok.copy()
    bad_sign[1, 0] = 0.5
    call("sign", thr=bad_sign)
    call("grid limit", G=1 << 30, H=721, W=1440, fc_bs=1 << 40, truth_bs=1 << 40)
    call("grid limit", G=1, S=16, src=np.tile(src_ok[:1], (16, 1)), thr=np.tile(thr_ok[:1], (16, 1)), C=3, H=1 << 28,
         W=4, M=32, T=tmax, fc_bs=1 << 40, truth_bs=1 << 40)              # the finishing kernel's grid
    # G == 0 does nothing and asks for nothing
    assert L.paradis_prob_update(None, 0, None, 0, None, None, 0, None, None, None, None, None, 0, 4, 2, 3, 2, 4, 8,
                                 None) == 0
