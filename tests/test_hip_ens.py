"""GPU: ensemble verification - the kernel pair ``paradis_ens_update`` through ``ensemble.EnsembleCard`` against the numpy
restatement tests/ens_oracle.py at its dispatch edges, its bit-level promises (vector path == scalar path, run == run,
two updates == one update of the concatenated ensembles, the running ordinal of the tie-breaking), two cross-checks and
the ``Forecaster.run(ensemble=...)`` hook.

Asserted per case (``_Judge`` prints and records both figures, as tests/test_hip_verify.py does):
  * the int64 accumulators (``nV``, rank histogram, ``n_samples``) equal the oracle's bit for bit;
  * each double row sum agrees with the oracle's float32-cell restatement within ``2 n 2^-53`` relative, ``n = G W`` the
    cells summed into the row: all four sums are of non-negative terms, and both sides sum the same fp32 terms in double,
    in different orders (each within ``(n - 1) 2^-53`` of the exact sum);
  * the reported metrics agree with the float64 oracle within the project's forward ceiling 1e-5, element by
    element.

Input design.  truth ~ N(0, 1); member i = truth + off_c + 0.8 (0.8 common + 0.6 e_i) with common, e_i ~ N(0, 1)
and |off_c| = 0.2: correlated, under-dispersive members with an offset (the truth reaches every rank).  The LAST channel is precipitation-like:
quantised to steps of 0.5 and clipped at 0, so that most of its cells are tied.  The first and last cell of every row
and the cells on both sides of every 128-cell boundary (every walk boundary of a wave: 256 cells, 128 in the 32-member
variant) carry 2^10 times the truth and the errors of the rest: a cell dropped or counted twice there moves every sum
by far more than any bound.  About 2 % of the cells hold a NaN, +Inf or -Inf in one member, another 2 % in the truth.
No subnormals.  Every design goes through the oracle on the CPU before the kernel is judged on it (``check_design``):
every rank bin of every channel is non-empty, at least half of the quantised channel's cells have ``eq > 0``,
``crps_fair >= 0.2 mae_members`` everywhere (the subtraction does not cancel), and 1 % .. 10 % of the cells are invalid.

Shapes come from ``paradis_ens_rows(W, M)`` and ``paradis_ens_max_members()``."""
import functools

import numpy as np
import pytest
import torch

from tests import ens_oracle as EO

pytestmark = pytest.mark.gpu
FWD = 1e-5
SPIKE = np.float32(1024.0)
BANDS = {"global": (-90.0, 90.0), "nh": (0.0, 90.0)}
SUMS = ("A", "P", "E2", "V")
METRICS = ("mae_members", "crps", "crps_fair", "rmse_mean", "spread", "spread_skill", "outliers", "rank_hist")


def _L():
    from paradis_model_amd import _lib
    return _lib.lib


def rows(W, M):
    return int(_L().paradis_ens_rows(W, M))


def mmax():
    return int(_L().paradis_ens_max_members())


def lat_deg(H):
    return np.linspace(-88.0, 88.0, H) if H > 1 else np.zeros(1)


def names_of(C):
    return [f"c{i}" for i in range(C)]


class _Judge:
    """collects a figure and its bound per quantity, prints and records them, asserts at the end"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad = record_property, case, []

    def add(self, name, figure, bound):
        print(f"ENS | {self.case} | {name} | {figure:.3e} | bound {bound:.3e}")
        self.rp(name, f"figure={figure:.3e} bound={bound:.3e}")
        if not figure <= bound:
            self.bad.append((name, figure, bound))

    def done(self):
        assert not self.bad, (self.case, self.bad)


# ================================================================================================ inputs
def spike_columns(W):
    return sorted({0, W - 1} | {b + d for b in range(128, W, 128) for d in (-1, 0)})


def design(seed, G, M, C, H, W, bad=True):
    """(forecast [G * M, C, H, W], truth [G, C, H, W]) float32 numpy, by the module docstring"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    y = rng.standard_normal((G, C, H, W)).astype(f32)
    common = rng.standard_normal((G, 1, C, H, W)).astype(f32)
    e = rng.standard_normal((G, M, C, H, W)).astype(f32)
    off = np.array([0.2 if c % 2 == 0 else -0.2 for c in range(C)], f32).reshape(1, 1, C, 1, 1)
    err = (off + f32(0.8) * (f32(0.8) * common + f32(0.6) * e)).astype(f32)
    x = (y[:, None] + err).astype(f32)
    if C >= 2:                                                 # the precipitation-like channel
        q = C - 1
        y[:, q] = np.clip(np.round(y[:, q] * 2) / 2, 0, None)
        x[:, :, q] = np.clip(np.round(x[:, :, q] * 2) / 2, 0, None)
    cols = spike_columns(W)
    y[..., cols] *= SPIKE
    x[..., cols] *= SPIKE
    if bad:
        n = G * C * H * W
        k = max(3, n // 50)
        cells = rng.permutation(n)[:2 * k]
        vals = (np.nan, np.inf, -np.inf)
        xf = x.transpose(0, 2, 3, 4, 1).reshape(n, M)          # a copy: written back below
        yf = y.reshape(n)
        for j, cell in enumerate(cells[:k]):
            xf[cell, rng.integers(M)] = vals[j % 3]
        for j, cell in enumerate(cells[k:]):
            yf[cell] = vals[j % 3]
        x = xf.reshape(G, C, H, W, M).transpose(0, 4, 1, 2, 3)
    x = np.ascontiguousarray(x, f32).reshape(G * M, C, H, W)
    tiny = np.finfo(f32).tiny
    for v in (x, y):
        fin = np.isfinite(v) & (v != 0)
        assert (np.abs(v[fin]) >= tiny).all()                  # no subnormals
    return x, np.ascontiguousarray(y)


def check_design(case, fc, truth, M, chan, band_w, quantised=None, n0=0, salt=0):
    """the oracle on the inputs, before they are relied on; returns (real32, ints, report64)"""
    real32, ints, detail = EO.row_sums(fc, truth, M, chan, n0, salt, np.float32)
    real64, ints64, _ = EO.row_sums(fc, truth, M, chan, n0, salt, np.float64)
    assert np.array_equal(ints, ints64)
    per_channel = ints[:, :, 1:].sum(axis=1)
    assert (per_channel > 0).all(), (case, "an empty rank bin", per_channel.tolist())
    cells = sum(t["valid"].size for t in detail.values())
    invalid = sum(int((~t["valid"]).sum()) for t in detail.values()) / cells
    assert 0.01 <= invalid <= 0.10, (case, "invalid fraction", invalid)
    tied = None
    if quantised is not None:
        ts = [t for (g, cs), t in detail.items() if cs == quantised]
        tied = sum(int((t["eq"][t["valid"]] > 0).sum()) for t in ts) / sum(int(t["valid"].sum()) for t in ts)
        assert tied >= 0.5, (case, "tied fraction", tied)
    rep = EO.report(real64, ints, band_w, M)
    ratio = rep["crps_fair"] / rep["mae_members"]
    assert (ratio >= 0.2).all(), (case, "crps_fair / mae_members", float(ratio.min()))
    print(f"ENS | {case} | invalid {invalid:.3f} | tied {tied} | crps_fair / mae >= {float(ratio.min()):.3f} | "
          f"smallest bin {int(per_channel.min())}")
    return real32, ints, rep


def place(fc, truth, M, layout):
    """device tensors holding ``fc`` / ``truth`` in the memory layout of the case"""
    B, C, H, W = fc.shape
    f, t = torch.from_numpy(fc), torch.from_numpy(truth)
    if layout == "dense":
        return f.cuda(), t.cuda()
    if layout == "offset":
        v = torch.zeros(f.numel() + 1, device="cuda")[1:].view(B, C, H, W)
        v.copy_(f)
        assert v.data_ptr() % 16 == 4
        return v, t.cuda()
    chunk = torch.full((B, 3, C, H, W), float("nan"), device="cuda")        # "views"
    true = torch.full((B, C, H, W), float("nan"), device="cuda")
    chunk[:, 1] = f.cuda()
    true[::M] = t.cuda()
    fv, tv = chunk[:, 1], true[::M]
    assert fv.stride(0) == 3 * C * H * W and (tv.shape[0] == 1 or tv.stride(0) == M * C * H * W)
    return fv, tv


def judge(J, card, lead, real32, ints, rep64, G, W, n_samples):
    """one lead of a card against the oracle's accumulators and report"""
    cnt = card.counts()
    assert cnt["valid"].dtype == np.int64 and cnt["rank_counts"].dtype == np.int64 and cnt["n_samples"].dtype == np.int64
    assert np.array_equal(cnt["valid"][lead], ints[..., 0]), "nV"
    assert np.array_equal(cnt["rank_counts"][lead], ints[..., 1:]), \
        ("histogram", np.argwhere(cnt["rank_counts"][lead] != ints[..., 1:])[:5].tolist())
    assert cnt["n_samples"].tolist() == n_samples
    got = cnt["sums"][lead]
    bound = 2.0 * G * W * 2.0 ** -53
    for k, name in enumerate(SUMS):
        ref = real32[..., k]
        err = np.abs(got[..., k] - ref) / np.where(ref > 0, ref, 1.0)
        assert (got[..., k][ref == 0] == 0).all(), name
        J.add(f"row sum {name}", float(err.max()), bound)
    res = card.result()
    for m in METRICS:
        ref = rep64[m]
        assert np.isfinite(ref).all() and res[m][lead].shape == ref.shape, m
        scale = np.where(ref != 0, np.abs(ref), 1.0)
        J.add(m, float((np.abs(res[m][lead] - ref) / scale).max()), FWD)
    assert np.abs(res["rank_hist"][lead].sum(axis=-1) - 1.0).max() <= 1e-12
    return res


# ================================================================================================ 1. the kernel pair
# name -> (G, M, C, H, W, layout, channels subset or None); M = 0: the library's maximum; H = 0: rows(W, M) + 1, a second
# workgroup that owns one row
CASES = {
    "M=2 W=4 rows+1":                 (1, 2, 2, 0, 4, "dense", None),
    "M=3 G=3 W=6 scalar":             (3, 3, 3, 5, 6, "dense", None),
    "M=5 G=3 W=68":                   (3, 5, 3, 3, 68, "dense", None),
    "M=5 G=3 W=68 offset (scalar)":   (3, 5, 3, 3, 68, "offset", None),
    "M=3 G=3 H=1 W=260":              (3, 3, 3, 1, 260, "dense", None),
    "M=8 W=4 rows+1":                 (1, 8, 2, 0, 4, "dense", None),
    "M=16 G=3 W=260 rows+1":          (3, 16, 3, 0, 260, "dense", None),
    "M=16 W=1440 H=3 views":          (1, 16, 2, 3, 1440, "views", None),
    "M=16 G=3 W=68 subset":           (3, 16, 4, 6, 68, "views", ("c3", "c0")),
    "M=max W=1440 H=3":               (1, 0, 2, 3, 1440, "dense", None),
    "M=max G=3 W=68 rows+1":          (3, 0, 3, 0, 68, "dense", None),
    "M=max G=3 W=6 scalar":           (3, 0, 2, 100, 6, "dense", None),
    "M=max W=260 offset (scalar)":    (1, 0, 2, 5, 260, "offset", None),
}


def resolve(case):
    G, M, C, H, W, layout, subset = CASES[case]
    M = M or mmax()
    H = H or rows(W, M) + 1
    assert G * M * C * H * W <= 2_100_000                      # member values of a case
    return G, M, C, H, W, layout, subset


@pytest.mark.parametrize("case", list(CASES))
def test_update_at_dispatch_edges(case, record_property):
    from paradis_model_amd.ensemble import EnsembleCard
    G, M, C, H, W, layout, subset = resolve(case)
    assert mmax() >= 16 and rows(W, M) >= 1
    fc, truth = design(500 + list(CASES).index(case), G, M, C, H, W)
    names = names_of(C)
    card = EnsembleCard(names, lat_deg(H), 2, M, bands=BANDS, channels=subset, seed=3)
    chan = card.index
    assert card.names == (list(subset) if subset else names) and card.all_names == names
    quantised = chan.index(C - 1) if (C - 1) in chan else None
    real32, ints, rep64 = check_design(case, fc, truth, M, chan, card.band_w, quantised, n0=0, salt=3 + 1)
    f, t = place(fc, truth, M, layout)
    before = (f.clone(), t.clone())
    card.update(1, f, t)
    assert torch.equal(f.nan_to_num(7.0), before[0].nan_to_num(7.0)) and \
        torch.equal(t.nan_to_num(7.0), before[1].nan_to_num(7.0))              # neither input is written
    J = _Judge(record_property, case)
    res = judge(J, card, 1, real32, ints, rep64, G, W, [0, G])
    J.done()
    assert res["count"].tolist() == [0, G] and res["members"] == M and res["bands"] == list(BANDS)
    assert all(np.isnan(res[m][0]).all() for m in METRICS)                    # the lead never updated
    assert int(card.acc_int[0].abs().sum()) == 0 and float(card.acc_real[0].abs().sum()) == 0.0


# ================================================================================================ 2. bit-level promises
def _equal(a, b):
    return torch.equal(a.acc_real, b.acc_real) and torch.equal(a.acc_int, b.acc_int) and \
        torch.equal(a.n_samples, b.n_samples)


@pytest.mark.parametrize("M", [5, 0])
def test_bit_level_promises(M, record_property):
    from paradis_model_amd.ensemble import EnsembleCard
    M = M or mmax()
    G, C, W = 3, 3, 260
    H = rows(W, M) + 1
    fc, truth = design(700 + M, G, M, C, H, W)
    names = names_of(C)

    def fresh(seed=0):
        return EnsembleCard(names, lat_deg(H), 2, M, bands=BANDS, seed=seed)

    fv, tv = place(fc, truth, M, "dense")
    fs, ts = place(fc, truth, M, "offset")
    a, b, c = fresh(), fresh(), fresh()
    a.update(0, fv, tv)
    b.update(0, fs, ts)
    c.update(0, fv, tv)
    assert _equal(a, b), "the scalar path and the vector path differ"
    assert _equal(a, c), "two runs differ"
    real32, ints, rep64 = check_design(f"promises M={M}", fc, truth, M, list(range(C)), a.band_w, C - 1)
    J = _Judge(record_property, f"promises M={M}")
    judge(J, a, 0, real32, ints, rep64, G, W, [G, 0])
    J.done()
    # two updates of G = 1 and G = 2 == one update of the three ensembles: doubles, integers and - through the running
    # ordinal - the ranks of the tied cells
    two = fresh()
    two.update(0, fv[:M], tv[:1])
    assert two.n_samples.tolist() == [1, 0]
    two.update(0, fv[M:], tv[1:])
    assert _equal(two, a)
    # the ordinal matters: the same two ensembles as a first update break their ties differently
    late, early = fresh(), fresh()
    late.update(0, fv[:M], tv[:1])
    late.update(0, fv[M:], tv[1:])
    early.update(0, fv[M:], tv[1:])
    early.update(0, fv[:M], tv[:1])
    assert torch.equal(late.acc_int[..., 0], early.acc_int[..., 0])           # the valid cells do not depend on it
    assert not torch.equal(late.acc_int, early.acc_int)
    # G == 0 leaves everything untouched
    keep = (two.acc_real.clone(), two.acc_int.clone())
    two.update(0, fv[:0], tv[:0])
    assert torch.equal(two.acc_real, keep[0]) and torch.equal(two.acc_int, keep[1]) and two.n_samples.tolist() == [G, 0]
    # reset() restarts the ordinal
    two.reset()
    assert int(two.acc_int.abs().sum()) == 0 and int(two.n_samples.sum()) == 0
    assert np.isnan(two.result()["crps"]).all()
    two.update(0, fv, tv)
    assert _equal(two, a)
    # another seed changes only the ranks of tied cells
    other = fresh(seed=11)
    other.update(0, fv, tv)
    assert torch.equal(other.acc_real, a.acc_real) and torch.equal(other.acc_int[..., 0], a.acc_int[..., 0])
    assert not torch.equal(other.acc_int, a.acc_int)
    want = EO.row_sums(fc, truth, M, list(range(C)), 0, 11, np.float32)[1]
    assert np.array_equal(other.counts()["rank_counts"][0], want[..., 1:])
    cont = list(range(C - 1))                                  # the continuous channels hold no tie: the same ranks
    assert torch.equal(other.acc_int[:, cont], a.acc_int[:, cont])
    # the lead enters the salt: the same update at lead 1 ranks the tied cells of the quantised channel differently
    a.update(1, fv, tv)
    assert torch.equal(a.acc_real[1], a.acc_real[0]) and torch.equal(a.acc_int[1][cont], a.acc_int[0][cont])
    assert not torch.equal(a.acc_int[1], a.acc_int[0])


def test_update_is_graph_capturable():
    """an update captured in a HIP graph and replayed twice equals two eager updates (the ordinal is read on the device)"""
    from paradis_model_amd.ensemble import EnsembleCard
    from paradis_model_amd.harness import capture_forward
    G, M, C, H, W = 2, 4, 2, 8, 64
    fc, truth = design(29, G, M, C, H, W)
    fd, td = torch.from_numpy(fc).cuda(), torch.from_numpy(truth).cuda()
    eager = EnsembleCard(names_of(C), lat_deg(H), 2, M)
    eager.update(1, fd, td)
    eager.update(1, fd, td)
    graphed = EnsembleCard(names_of(C), lat_deg(H), 2, M)
    graph, _ = capture_forward(lambda: graphed.update(1, fd, td), warmup=1)
    torch.cuda.synchronize()
    graphed.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(graphed, eager) and graphed.n_samples.tolist() == [0, 2 * G]


def test_update_refusals_on_the_device():
    from paradis_model_amd.ensemble import EnsembleCard
    H, W, M = 4, 8, 2
    card = EnsembleCard(names_of(2), lat_deg(H), 1, M)
    x, y = torch.zeros(4, 2, H, W, device="cuda"), torch.zeros(2, 2, H, W, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        card.update(0, x.cpu(), y)
    with pytest.raises(ValueError, match="dense"):
        card.update(0, torch.zeros(4, 2, H, 2 * W, device="cuda")[..., ::2], y)
    with pytest.raises(ValueError, match="whole ensembles"):
        card.update(0, x[:3], y)
    cpu_card = EnsembleCard(names_of(2), lat_deg(H), 1, M, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu_card.update(0, x, y)
    assert int(card.acc_int.abs().sum()) == 0


# ================================================================================================ 3. cross-checks
def test_identical_members_give_the_scorecards_numbers():
    """an ensemble whose members all equal one forecast f: crps == mae_members, spread == 0 and rmse_mean / crps equal to
    Scorecard's rmse / mae on f (the same latitude weights, one global band, all cells valid).  M = 4: the mean of four
    equal values is exact."""
    from paradis_model_amd.ensemble import EnsembleCard
    from paradis_model_amd.verify import Scorecard
    from tests.test_hip_verify import lat_weights
    G, M, C, H, W = 2, 4, 3, 9, 68
    rng = np.random.default_rng(41)
    t = rng.standard_normal((G, C, H, W)).astype(np.float32)
    f = (t + np.float32(0.7) * rng.standard_normal((G, C, H, W)).astype(np.float32) + np.float32(0.2)).astype(np.float32)
    w = lat_weights(H)
    fd, td = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    members = fd.repeat_interleave(M, dim=0)
    card = EnsembleCard(names_of(C), lat_deg(H), 1, M, weights=w)
    card.update(0, members, td)
    res = card.result()
    score = Scorecard(names_of(C), w, 1)
    score.update(0, fd, td)
    ref = score.result()
    assert np.array_equal(res["crps"], res["mae_members"]) and (res["spread"] == 0).all()
    assert (card.counts()["valid"] == G * W).all()
    for mine, theirs in (("rmse_mean", "rmse"), ("crps", "mae")):
        e = np.abs(res[mine][0, :, 0] - ref[theirs][0]) / np.abs(ref[theirs][0])
        print(f"ENS | identical members | {mine} vs {theirs} | {float(e.max()):.3e}")
        assert e.max() <= FWD, (mine, float(e.max()))


@pytest.mark.parametrize("M", [3, 16])
def test_all_tied_state_ranks_by_the_hash(M):
    """x_i = y everywhere: eq = M, the histogram is the oracle's hash ranks exactly, the CRPS is 0 and - where the fp32
    mean of M equal values is exact - every score"""
    from paradis_model_amd.ensemble import EnsembleCard
    G, C, H, W = 2, 2, 5, 260
    rng = np.random.default_rng(43)
    y = (np.round(rng.standard_normal((G, C, H, W)) * 64) / 64).astype(np.float32)    # short dyadic values: M y is exact
    x = np.ascontiguousarray(np.repeat(y, M, axis=0))
    card = EnsembleCard(names_of(C), lat_deg(H), 1, M, seed=5)
    card.update(0, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    _, ints, detail = EO.row_sums(x, y, M, [0, 1], 0, 5, np.float32)
    assert all((t["eq"] == M).all() and (t["lo"] == 0).all() for t in detail.values())
    cnt = card.counts()
    assert np.array_equal(cnt["rank_counts"][0], ints[..., 1:]) and (cnt["valid"] == G * W).all()
    assert (ints[..., 1:].sum(axis=(0, 1)) > 0).all()           # the hash reaches every rank
    res = card.result()
    assert (res["crps"] == 0).all() and (res["mae_members"] == 0).all() and (res["crps_fair"] == 0).all()
    if M & (M - 1) == 0:                                       # (1.0f / M is exact: so is the mean of M equal values)
        assert float(card.acc_real.abs().sum()) == 0.0 and (res["rmse_mean"] == 0).all() and (res["spread"] == 0).all()


# ================================================================================================ 4. the forecaster hook
@functools.lru_cache(None)
def _rollout_setup():
    from paradis_model_amd.config import feature_layout, reduced_config, stub_datamodule
    from paradis_model_amd.forecast import PostSpec
    from paradis_model_amd.model import Paradis
    from tests import forecast_oracle as FO
    from tests._util import make_grid, seeded
    H, W, B, S = 32, 64, 4, 2
    cfg = reduced_config()
    _, lg, og = make_grid(H, W, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda().eval()
    names = list(feature_layout(cfg).output_name_order)
    levels = list(cfg.features.pressure_levels)
    mean, std = FO.channel_stats(names)
    _, _, zs = FO.classes(names, True)
    spec = PostSpec.from_features(names, levels, zscore_mean=mean[zs], zscore_std=std[zs], q_min=FO.Q_MIN,
                                  q_max=FO.Q_MAX, custom_normalization=True)
    lat, lon = FO.grid_deg(H, W, False)
    inputs = (seeded(177, B, 1, 166, H, W).cuda(), seeded(179, B, S, H, W, 10, kind="rand").cuda(),
              seeded(180, B, 1, H, W, 10).cuda())
    return model, spec, lat, lon, inputs, (H, W, B, S)


def test_forecaster_hook():
    """run(ensemble=card, ...) beside a scorecard at 32x64 with B = 4, M = 2: the card equals ``card.update`` called by
    hand on the stored chunk with the truth of each ensemble's first member, and the scorecard's numbers are those of a
    run without the card"""
    from paradis_model_amd.ensemble import EnsembleCard
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.verify import Scorecard
    from tests import forecast_oracle as FO
    from tests.test_hip_verify import _Collect, lat_weights
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    C, M = spec.num_channels, 2
    norm = FO.normalised_state(31, spec.names, B, S, C, H, W).cuda()
    phys = torch.empty(B, S, C, H, W, device="cuda")
    for s in range(S):
        postprocess(norm[:, s], spec, lat, lon, phys, s)
    chosen = [spec.names[-1], spec.names[0], spec.names[5]]

    def fresh():
        return EnsembleCard(spec.names, lat, S, M, channels=chosen, bands=BANDS, seed=2)

    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=True)
    card, score = fresh(), Scorecard(spec.names, lat_weights(H), S)
    seen = _Collect()
    fc.run(*inputs, seen, ensemble=card, scorecard=score, truth=phys)
    states = torch.cat([c[1] for c in seen.chunks], dim=1)                     # [B, S, C, H, W] as the writer saw them
    by_hand = fresh()
    for s in range(S):
        by_hand.update(s, states[:, s].cuda(), phys[::M, s])
    assert _equal(card, by_hand) and card.n_samples.tolist() == [B // M] * S
    assert (card.counts()["valid"] == (B // M) * W).all()
    res = card.result()
    assert np.isfinite(res["crps_fair"]).all() and (res["spread"] > 0).all()
    alone = Scorecard(spec.names, lat_weights(H), S)
    fc.run(*inputs, None, scorecard=alone, truth=phys)
    assert torch.equal(score.acc, alone.acc)
    only = fresh()
    fc.run(*inputs, None, ensemble=only, truth=phys)                           # without the other tables
    assert _equal(only, card)
    with pytest.raises(ValueError, match="whole ensembles"):
        fc.run(*inputs, None, ensemble=EnsembleCard(spec.names, lat, S, 3), truth=phys)
    with pytest.raises(ValueError, match="ensemble card needs truth"):
        fc.run(*inputs, None, ensemble=card)
    with pytest.raises(ValueError, match="leads"):
        fc.run(*inputs, None, ensemble=EnsembleCard(spec.names, lat, S - 1, M), truth=phys)
    assert _equal(card, by_hand)
