"""Host side of the ensemble verification, no GPU: the numpy oracle's own closed forms (tests/ens_oracle.py), the argument
checks and host arithmetic of ``ensemble.EnsembleCard`` on ``device="cpu"``, the ``Forecaster.run(ensemble=...)``
refusals and the C ABI's refusals before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from paradis_model_amd import ensemble as EN
from tests import ens_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tp", "u10", "v10", "t2m"]
LAT = np.linspace(-80.0, 80.0, 5)
SYMBOLS = ("paradis_ens_max_members", "paradis_ens_rows", "paradis_ens_ws_bytes", "paradis_ens_update")
F32 = np.float32


def one_row(x, y, M, dtype=np.float64):
    """members ``x [M, W]`` and truth ``y [W]`` as a one-channel, one-row update -> (real, ints, report with weight 1)"""
    fc = np.asarray(x, F32).reshape(M, 1, 1, -1)
    tr = np.asarray(y, F32).reshape(1, 1, 1, -1)
    real, ints, detail = EO.row_sums(fc, tr, M, [0], 0, 0, dtype)
    return real, ints, EO.report(real, ints, np.ones((1, 1)), M), detail[(0, 0)]


# ================================================================================================ 1. the oracle itself
def test_oracle_two_members_closed_form():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 50))
    y = rng.standard_normal(50)
    _, _, rep, _ = one_row(x, y, 2)
    x, y = x.astype(F32).astype(np.float64), y.astype(F32).astype(np.float64)
    want = np.mean((np.abs(x[0] - y) + np.abs(x[1] - y)) / 2 - np.abs(x[0] - x[1]) / 2)
    assert abs(rep["crps_fair"][0, 0] - want) <= 1e-14 * abs(want)
    want_own = np.mean((np.abs(x[0] - y) + np.abs(x[1] - y)) / 2 - np.abs(x[0] - x[1]) / 4)
    assert abs(rep["crps"][0, 0] - want_own) <= 1e-14 * abs(want_own)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_small_integer_offsets_are_exact(dtype):
    y = np.array([3.0, -7.0, 0.5], F32)
    d = np.array([-2, 0, 1, 5], F32)                           # M = 4: the mean is exact
    x = y[None, :] + d[:, None]
    t = EO.cell_terms(x, y, dtype)
    assert t["A"].dtype == dtype
    assert (t["A"] == 8).all() and (t["P"] == (2 + 3 + 7 + 1 + 5 + 4)).all()
    assert (t["E2"] == 1.0).all()                              # mean offset 1
    assert (t["V"] == 9 + 1 + 0 + 16).all()
    assert (t["lo"] == 1).all() and (t["eq"] == 1).all() and t["valid"].all()


def test_oracle_all_members_equal_the_truth():
    y = np.array([1.5, -2.25, 0.0, 1024.0], F32)               # short dyadic values: M y and its partial sums are exact
    for M in (2, 3, 4, 5, 16):
        t = EO.cell_terms(np.repeat(y[None], M, axis=0), y, np.float32)
        exact_mean = M & (M - 1) == 0                          # (1.0f / M is exact for a power of two only)
        assert all((t[k] == 0).all() for k in (("A", "P", "E2", "V") if exact_mean else ("A", "P"))), M
        assert (t["eq"] == M).all() and (t["lo"] == 0).all()
        r = EO.ranks(t["lo"].reshape(1, -1), t["eq"].reshape(1, -1), 0, 0, 1, 0)
        assert ((r >= 0) & (r <= M)).all()


def test_oracle_pair_sum_is_the_sorted_identity():
    rng = np.random.default_rng(2)
    for M in (2, 3, 5, 16, 32):
        x = rng.standard_normal((M, 40)).astype(F32)
        t = EO.cell_terms(x, np.zeros(40, F32), np.float64)
        xs = np.sort(x.astype(np.float64), axis=0)
        want = ((2 * np.arange(M) - M + 1)[:, None] * xs).sum(axis=0)
        assert np.abs(t["P"] - want).max() <= 1e-12 * np.abs(want).max(), M


def test_oracle_crps_is_at_most_the_members_mae_and_the_histogram_sums_to_one():
    rng = np.random.default_rng(3)
    for M in (2, 5, 16):
        x = rng.standard_normal((M, 300)) * 0.7 + 0.3
        y = np.round(rng.standard_normal(300) * 2) / 2            # ties among the members? none; in the truth: no matter
        _, ints, rep, _ = one_row(x, y, M)
        assert rep["crps"][0, 0] <= rep["mae_members"][0, 0] and rep["crps_fair"][0, 0] <= rep["crps"][0, 0]
        assert abs(rep["rank_hist"][0, 0].sum() - 1.0) <= 1e-15 and ints[0, 0, 1:].sum() == ints[0, 0, 0] == 300


def test_oracle_calibrated_gaussian_ensemble():
    """truth and members drawn from one distribution per cell: spread_skill near 1, a flat rank histogram"""
    rng = np.random.default_rng(4)
    M, n = 8, 40000
    centre = rng.standard_normal(n)
    x = centre[None] + rng.standard_normal((M, n))
    y = centre + rng.standard_normal(n)
    _, ints, rep, _ = one_row(x, y, M)
    assert 0.9 <= rep["spread_skill"][0, 0] <= 1.1
    hist = ints[0, 0, 1:]
    p = 1.0 / (M + 1)
    sigma = np.sqrt(n * p * (1 - p))
    assert np.abs(hist - n * p).max() <= 5 * sigma              # five sigma of a binomial count
    assert abs(rep["outliers"][0, 0] - 2 * p) <= 0.01


def test_oracle_hash_and_ordinal():
    assert EO.hash32(np.array([0, 1], np.uint32)).tolist() == [0, 1753845952]
    lo, eq = np.zeros((2, 3), np.int64), np.full((2, 3), 4, np.int64)
    a = EO.ranks(lo, eq, 0, 1, 2, 0)
    b = EO.ranks(lo, eq, 1, 1, 2, 0)
    assert not np.array_equal(a, b) and np.array_equal(a, EO.ranks(lo, eq, 2 ** 32, 1, 2, 2 ** 32))
    y = np.zeros((3, 1, 2, 3), F32)
    x = np.zeros((12, 1, 2, 3), F32)
    whole = EO.row_sums(x, y, 4, [0], 0, 7)[1]
    parts = EO.row_sums(x[:4], y[:1], 4, [0], 0, 7)[1] + EO.row_sums(x[4:], y[1:], 4, [0], 1, 7)[1]
    assert np.array_equal(whole, parts)


def test_oracle_invalid_cells_add_nothing():
    x = np.ones((3, 6), F32)
    y = np.zeros(6, F32)
    x[1, 0], x[2, 1], y[2], y[3] = np.nan, np.inf, -np.inf, np.nan
    real, ints, _, _ = one_row(x, y, 3)
    assert ints[0, 0, 0] == 2 and ints[0, 0, 1:].tolist() == [2, 0, 0, 0]
    assert real[0, 0].tolist() == [6.0, 0.0, 2.0, 0.0]


# ================================================================================================ 2. EnsembleCard on the host
def _card(**kw):
    kw.setdefault("bands", {"nh": (20, 90), "global": (-90, 90)})
    kw.setdefault("members", 4)
    return EN.EnsembleCard(NAMES, LAT, 2, device="cpu", **kw)


def test_card_shapes_and_subset():
    e = _card(channels=["t2m", "tp"], seed=9)
    assert EN.max_members() >= 16
    assert e.names == ["t2m", "tp"] and e.all_names == NAMES and e.index == [3, 0] and e._chan.tolist() == [3, 0]
    assert e.acc_real.shape == (2, 2, 5, 4) and e.acc_real.dtype == torch.float64
    assert e.acc_int.shape == (2, 2, 5, 6) and e.acc_int.dtype == torch.int64 and e.n_samples.dtype == torch.int64
    assert e._rM == 0.25 and e.members == 4 and e.seed == 9 and not e.TAKES_CLIM_INDEX
    assert _card(members=3)._rM == float(F32(1) / F32(3))
    assert e.band_w.shape == (2, 5) and e.band_w[0, :3].tolist() == [0.0, 0.0, 0.0]
    # about 0.5 GB for 40 leads of 96 channels at 721 rows with M = 16
    assert 40 * 96 * 721 * (4 + 2 + 16) * 8 == 487_280_640


def test_card_constructor_errors():
    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            _card(**kw)

    for m in (1, 0, EN.max_members() + 1, 2.5, True):
        bad("members must be", members=m)
    bad("seed", seed=-1)
    bad("seed", seed=1.5)
    bad("not among the names", channels=["q700"])
    bad("repeat", channels=["tp", "tp"])
    bad("at least one", channels=[])
    bad("EnsembleCard: band 'x'", bands={"x": (10, -10)})
    bad("bands must be", bands={})
    bad("weights", weights=torch.ones(4))
    for n_leads in (0, 1.5, True):
        with pytest.raises(ValueError, match="n_leads"):
            EN.EnsembleCard(NAMES, LAT, n_leads, 4, device="cpu")
    with pytest.raises(ValueError, match="lat_deg"):
        EN.EnsembleCard(NAMES, [0.0, 91.0], 1, 4, device="cpu")
    with pytest.raises(ValueError, match="names must list"):
        EN.EnsembleCard([], LAT, 1, 4, device="cpu")


def test_card_update_argument_errors_on_cpu_tensors():
    e = _card()
    f, t = torch.zeros(8, 4, 5, 8), torch.zeros(2, 4, 5, 8)

    def bad(match, lead=0, fc=f, truth=t, exc=ValueError):
        with pytest.raises(exc, match=match):
            e.update(lead, fc, truth)

    bad("lead", lead=2)
    bad("lead", lead=True)
    bad("float32", fc=f.double())
    bad("float32", truth=t.double())
    bad(r"\[B, C, H, W\]", truth=t[0])
    bad("the card has 4 channels and 5 latitudes", fc=torch.zeros(8, 3, 5, 8))
    bad("7 states are not whole ensembles of 4 members", fc=f[:7])
    bad("2 ensembles of 4 members need truth", truth=torch.zeros(8, 4, 5, 8))
    bad("truth is", truth=torch.zeros(2, 4, 5, 6))
    bad("forecast must hold dense", fc=torch.zeros(8, 4, 5, 16)[..., ::2])
    bad("truth must hold dense", truth=torch.zeros(2, 4, 5, 16)[..., ::2])
    bad("MI355X", exc=RuntimeError)                                      # every host check passed: the device check
    bad("MI355X", fc=torch.zeros(16, 3, 4, 5, 8)[:, 1], truth=torch.zeros(16, 4, 5, 8)[::4], exc=RuntimeError)


def _filled():
    """a card whose accumulators are filled by hand with the oracle's rows of two updates at lead 0"""
    M = 4
    e = _card(channels=["v10", "tp"], members=M)
    rng = np.random.default_rng(7)
    real = np.zeros((2, 5, 4))
    ints = np.zeros((2, 5, 2 + M), np.int64)
    n = 0
    for G in (2, 1):
        t = rng.standard_normal((G, 4, 5, 8)).astype(F32)
        f = (np.repeat(t, M, axis=0) + rng.standard_normal((G * M, 4, 5, 8)) * 0.5).astype(F32)
        f[0, 2, 2, 1] = np.nan
        r, i, _ = EO.row_sums(f, t, M, e.index, n, 0, np.float64)
        real, ints, n = real + r, ints + i, n + G
    e.acc_real[0] = torch.from_numpy(real)
    e.acc_int[0] = torch.from_numpy(ints)
    e.n_samples[0] = n
    return e, real, ints


def test_card_result_from_hand_filled_accumulators():
    e, real, ints = _filled()
    cnt = e.counts()
    assert np.array_equal(cnt["sums"][0], real) and np.array_equal(cnt["valid"][0], ints[..., 0])
    assert np.array_equal(cnt["rank_counts"][0], ints[..., 1:]) and cnt["n_samples"].tolist() == [3, 0]
    assert cnt["valid"].dtype == np.int64 and cnt["rank_counts"].dtype == np.int64 and cnt["sums"].dtype == np.float64
    assert cnt["valid"][0, 0, 2] == 3 * 8 - 2                            # the NaN cell of channel v10, in both updates
    res = e.result()
    want = EO.report(real, ints, e.band_w, 4)
    for k in EN.METRICS + ("rank_hist",):
        got = res[k]
        assert got.dtype == np.float64 and got.shape[:3] == (2, 2, 2), k
        assert np.isfinite(got[0]).all() and np.isnan(got[1]).all(), k   # lead 1 was never updated
        assert np.abs(got[0] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    assert res["rank_hist"].shape == (2, 2, 2, 5) and np.abs(res["rank_hist"][0].sum(-1) - 1).max() <= 1e-15
    assert (res["crps_fair"][0] <= res["crps"][0]).all() and (res["crps"][0] <= res["mae_members"][0]).all()
    assert np.array_equal(res["outliers"][0], res["rank_hist"][0, ..., 0] + res["rank_hist"][0, ..., 4])
    assert res["count"].tolist() == [3, 0] and res["names"] == ["v10", "tp"] and res["bands"] == ["nh", "global"]
    assert res["members"] == 4
    e.reset()
    assert float(e.acc_real.abs().sum()) == 0 and int(e.acc_int.abs().sum()) == 0 and int(e.n_samples.sum()) == 0
    assert np.isnan(e.result()["crps"]).all()


def test_card_sync_dist_makes_one_all_reduce(tmp_path, monkeypatch):
    import torch.distributed as dist
    e, _, _ = _filled()
    want = e.result()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        calls = []
        real = dist.all_reduce
        monkeypatch.setattr(dist, "all_reduce", lambda t, **kw: (calls.append((tuple(t.shape), t.dtype)), real(t, **kw))[1])
        got = e.result(sync_dist=True)
        assert calls == [((e.acc_real.numel() + e.acc_int.numel() + 2,), torch.float64)]
    finally:
        dist.destroy_process_group()
    for k in EN.METRICS + ("rank_hist", "count"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_card_prints():
    e, _, _ = _filled()
    res = e.result()
    text = EN.EnsembleCard.table(res, "tp")
    lines = text.split("\n")
    assert lines[0] == "tp / global / 4 members"
    assert lines[1].split() == ["lead", "count"] + list(EN.METRICS)
    assert lines[2].split()[:2] == ["0", "3"] and lines[3].split() == ["1", "0"] + ["nan"] * 7
    assert float(lines[2].split()[3]) == pytest.approx(res["crps"][0, 1, 1], rel=1e-4)
    assert lines[4] == "" and lines[5].split() == ["rank", "count", "0", "1", "2", "3", "4"]
    assert sum(float(v) for v in lines[6].split()[2:]) == pytest.approx(1.0, abs=1e-3)
    assert lines[7].split() == ["1", "0"] + ["nan"] * 5 and len(lines) == 8
    assert len({len(ln) for ln in lines[1:4]}) == 1 and len({len(ln) for ln in lines[5:]}) == 1     # aligned columns
    assert EN.EnsembleCard.table(res, "v10", band="nh").split("\n")[0] == "v10 / nh / 4 members"
    assert EN.EnsembleCard.table(res, "v10", band=None).split("\n")[0] == "v10 / nh / 4 members"
    for kw, word in ((dict(channel="u10"), "u10"), (dict(channel="tp", band="sh"), "sh")):
        with pytest.raises(ValueError, match=word):
            EN.EnsembleCard.table(res, **kw)


# ================================================================================================ 3. the forecaster hook
def test_forecaster_run_refusals_with_an_ensemble_card():
    from paradis_model_amd.forecast import Forecaster, PostSpec
    from paradis_model_amd.verify import Scorecard
    H, W = 5, 8
    names = NAMES[:3]
    spec = PostSpec.from_features(names, [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    fc = Forecaster(None, spec, LAT, np.zeros(W), graph=False)
    inp, forc, const = torch.zeros(4, 1, 6, H, W), torch.zeros(4, 2, H, W, 1), torch.zeros(4, 1, H, W, 1)
    card = lambda n=2, nm=names, m=2: EN.EnsembleCard(nm, LAT, n, m, device="cpu")     # noqa: E731
    with pytest.raises(ValueError) as e:
        fc.run(inp, forc, const, None, ensemble=card(), truth=None)
    assert str(e.value) == "Forecaster.run: an ensemble card needs truth [B, n_stored, C, H, W] on the device"
    good = torch.zeros(4, 2, 3, H, W)
    kw = dict(scorecard=None, truth=good, truth_normalized=False, clim_index=None, B=4, n_stored=2, C=3, H=H, W=W)
    with pytest.raises(ValueError, match="truth must be float32"):
        fc._check_verification(**{**kw, "truth": good[:, :1]}, ensemble=card())
    with pytest.raises(ValueError) as e:
        fc._check_verification(**kw, ensemble=card(1))
    assert str(e.value) == "Forecaster.run: the ensemble card has 1 leads, the rollout stores 2"
    with pytest.raises(ValueError) as e:
        fc._check_verification(**kw, ensemble=card(2, ["tp", "v10", "u10"]))
    assert str(e.value) == "Forecaster.run: the ensemble card's names are not the chunk's channel names (PostSpec.names)"
    with pytest.raises(ValueError) as e:
        fc._check_verification(**kw, ensemble=card(m=3))
    assert str(e.value) == "Forecaster.run: the ensemble card has 3 members, a batch of 4 states is not whole ensembles"
    with pytest.raises(ValueError, match="clim_index goes with a scorecard"):         # the card takes no clim_index
        fc._check_verification(**{**kw, "clim_index": torch.zeros(4, 2, dtype=torch.int32)}, ensemble=card())
    # the scorecard speaks first, the card last
    with pytest.raises(ValueError, match="the scorecard has 1 leads"):
        fc._check_verification(**{**kw, "scorecard": Scorecard(names, np.ones(H), 1, device="cpu")}, ensemble=card(1))
    with pytest.raises(RuntimeError, match="MI355X"):                   # every host check passed: the device check
        fc._check_verification(**kw, ensemble=card())
    with pytest.raises(ValueError, match="scorecard"):                  # as before: truth alone goes with nothing
        fc._check_verification(**kw)


# ================================================================================================ 4. the C ABI
def test_ens_symbols_are_declared_exported_and_bound():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    sig = _lib.SIGNATURES["paradis_ens_update"][1]
    assert len(sig) == 18 and sig[1] is ctypes.c_int64 and sig[3] is ctypes.c_int64 and sig[5] is ctypes.c_float
    assert sig[6] is ctypes.c_uint and _lib.SIGNATURES["paradis_ens_ws_bytes"][0] is ctypes.c_size_t
    L = _lib.lib
    assert L.paradis_abi_version() == 10
    mmax = L.paradis_ens_max_members()
    assert mmax >= 16 and EN.max_members() == mmax
    for W in (1, 4, 6, 64, 68, 260, 1440, 100000):
        for M in (2, 3, 5, 8, 16, mmax):
            assert L.paradis_ens_rows(W, M) >= 1, (W, M)
    assert L.paradis_ens_rows(64, 2) >= L.paradis_ens_rows(64, mmax)
    assert L.paradis_ens_rows(0, 4) == 0 and L.paradis_ens_rows(64, 1) == 0 and L.paradis_ens_rows(64, mmax + 1) == 0
    with open(os.path.join(ROOT, "paradis_model_amd", "csrc", "Makefile")) as f:
        assert "FLAGS_ensemble := -ffp-contract=off" in f.read()


def test_ens_workspace_holds_the_partials():
    """double [G][Cs][H][4], then uint32 [G][Cs][H][2 + M]; 0 for empty shapes"""
    from paradis_model_amd import _lib
    L = _lib.lib
    for (G, Cs, H, W, M) in ((2, 3, 32, 64, 4), (1, 96, 721, 1440, 16), (5, 1, 1, 64, 2)):
        assert L.paradis_ens_ws_bytes(G, Cs, H, W, M) == G * Cs * H * (32 + 4 * (2 + M))
    for shape in ((0, 3, 32, 64, 4), (2, 0, 32, 64, 4), (2, 3, 0, 64, 4), (2, 3, 32, 0, 4), (2, 3, 32, 64, 1),
                  (2, 3, 32, 64, L.paradis_ens_max_members() + 1), (-1, 3, 32, 64, 4)):
        assert L.paradis_ens_ws_bytes(*shape) == 0


def test_ens_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first

    def call(word, fc=fake, truth=fake, chan=fake, real=fake, ints=fake, n=fake, ws=fake, G=2, M=4, C=3, Cs=2, H=4, W=8,
             fc_bs=96, truth_bs=96):
        rc = L.paradis_ens_update(fc, fc_bs, truth, truth_bs, chan, 0.25, 0, real, ints, n, ws, G, M, C, Cs, H, W, None)
        assert rc == 1 and word in _lib.last_error(), (word, rc, _lib.last_error())

    call("bad shape", G=-1)
    call("bad shape", C=0)
    call("bad shape", Cs=0)
    call("bad shape", H=0)
    call("bad shape", W=0)
    call("members", M=1)
    call("members", M=0)
    call("members", M=L.paradis_ens_max_members() + 1)
    call("strides", fc_bs=95)
    call("strides", truth_bs=95)
    call("missing", real=None)
    call("missing", ints=None)
    call("missing", n=None)
    call("missing", ws=None)
    call("null input", fc=None)
    call("null input", truth=None)
    call("null input", chan=None)
    call("too large", H=1 << 16, W=1 << 15, fc_bs=1 << 40, truth_bs=1 << 40)
    call("grid limit", G=1 << 30, H=721, W=1440, fc_bs=1 << 40, truth_bs=1 << 40)
    call("grid limit", G=1, Cs=1 << 20, C=1 << 20, H=1 << 18, W=4, M=L.paradis_ens_max_members(), fc_bs=1 << 40,
         truth_bs=1 << 40)                                               # the finishing kernel's grid
    # G == 0 does nothing and asks for nothing
    assert L.paradis_ens_update(None, 0, None, 0, None, 0.25, 0, None, None, None, None, 0, 4, 3, 2, 4, 8, None) == 0
