"""GPU: probabilistic event verification - the kernel pair ``paradis_prob_update`` through
``probability.ProbabilityTable`` against the numpy restatement tests/prob_oracle.py at its dispatch edges, its bit-level
promises (vector path == scalar path, run == run, two updates == one update of the concatenated ensembles, a captured
update replayed, batch-strided views, an ensemble without a climatology slot), two cross-checks against
``events.EventTable`` and the ``Forecaster.run(probability=...)`` hook.

Asserted per case (``_Judge`` prints and records figure and bound, as tests/test_hip_ens.py does):
  * every int64 accumulator (``nV``, the joint histograms) and ``n_samples`` equals the oracle's bit for bit;
  * ``sum_{o,k} joint[j][o][k] == nV`` for every threshold of every source;
  * every reported value agrees with the oracle's float64 report within the project's forward ceiling 1e-5,
    element by element, NaN where the oracle has NaN.

Input design (tests/test_hip_ens.py's recipe).  Five channels; truth ~ N(0, 1); member i = truth + 0.8 (0.8 common +
0.6 e_i) with common, e_i ~ N(0, 1): correlated, under-dispersive members, so that the truth falls outside the whole
ensemble often enough to fill the corner bins.  The LAST channel is precipitation-like: quantised to steps of 0.5 and
clipped at 0.  About 2 % of the cells hold a NaN, +Inf or -Inf in one member, another 2 % in the truth; the climatology
(K = 2 slots, 0.3 N(0, 1)) holds a few NaN cells in the anomaly's channel.  Four sources: ``warm`` plain ``"ge"`` with 1
threshold, ``wind`` speed with 2, ``anom`` anomaly with 8 (not sorted), ``dry`` plain ``"le"`` with 3 on the quantised
channel; their thresholds sit at the 0.16, 0.5, 0.69 and 0.93 quantiles of the source's truth values (the 8-threshold
source adds 0.07, 0.31, 0.84 and 0.98), computed by the oracle.  Every design goes through the oracle on the CPU before
the kernel is judged on it (``check_design``): 1 % .. 10 % of the cells of every source are invalid, every threshold has
a truth event and a truth non-event, at the median threshold every one of the ``2 (M + 1)`` bins of every source is
non-empty; the ``M = 32`` cases have at least 2,340 cells per source, every other case at least 640.  The tiny grids
(3 x 2, 1 x 1) are exempt from the bin condition and compared on the integers alone.

Shapes come from ``paradis_prob_rows(W)`` and ``paradis_prob_max_members()``."""
import numpy as np
import pytest
import torch

from tests import prob_oracle as PO

pytestmark = pytest.mark.gpu
FWD = 1e-5
C = 5
BANDS = {"global": (-90.0, 90.0), "nh": (0.0, 90.0)}
NAMES = [f"c{i}" for i in range(C)]
# label -> (source for the table, oracle kind, c0, c1, direction, quantiles, index of the median threshold)
SOURCES = {"warm": ("c0", "plain", 0, 0, "ge", (0.5,), 0),
           "wind": (("speed", "c1", "c2"), "speed", 1, 2, "ge", (0.5, 0.93), 0),
           "anom": (("anomaly", "c3"), "anomaly", 3, 0, "ge", (0.93, 0.5, 0.16, 0.69, 0.07, 0.98, 0.31, 0.84), 1),
           "dry": ("c4", "plain", 4, 0, "le", (0.16, 0.5, 0.69), 1)}


def _L():
    from paradis_model_amd import _lib
    return _lib.lib


def rows(W):
    return int(_L().paradis_prob_rows(W))


def mmax():
    return int(_L().paradis_prob_max_members())


def lat_deg(H):
    return np.linspace(-88.0, 88.0, H) if H > 1 else np.zeros(1)


class _Judge:
    """collects a figure and its bound per quantity, prints and records them, asserts at the end"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad = record_property, case, []

    def add(self, name, figure, bound):
        print(f"PROB | {self.case} | {name} | {figure:.3e} | bound {bound:.3e}")
        self.rp(name, f"figure={figure:.3e} bound={bound:.3e}")
        if not figure <= bound:
            self.bad.append((name, figure, bound))

    def done(self):
        assert not self.bad, (self.case, self.bad)


# ================================================================================================ inputs
def design(seed, G, M, H, W, bad=True):
    """(forecast [G * M, C, H, W], truth [G, C, H, W], climatology [2, C, H, W], clim_index [G]) float32 / int32 numpy,
    by the module docstring"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    y = rng.standard_normal((G, C, H, W)).astype(f32)
    common = rng.standard_normal((G, 1, C, H, W)).astype(f32)
    e = rng.standard_normal((G, M, C, H, W)).astype(f32)
    x = (y[:, None] + f32(0.8) * (f32(0.8) * common + f32(0.6) * e)).astype(f32)
    q = C - 1                                                  # the precipitation-like channel
    y[:, q] = np.clip(np.round(y[:, q] * 2) / 2, 0, None)
    x[:, :, q] = np.clip(np.round(x[:, :, q] * 2) / 2, 0, None)
    clim = (f32(0.3) * rng.standard_normal((2, C, H, W))).astype(f32)
    if bad:
        n = G * C * H * W
        k = max(1, n // 50)
        cells = rng.permutation(n)[:2 * k]
        vals = (np.nan, np.inf, -np.inf)
        xf = x.transpose(0, 2, 3, 4, 1).reshape(n, M)          # a copy: written back below
        yf = y.reshape(n)
        for j, cell in enumerate(cells[:k]):
            xf[cell, rng.integers(M)] = vals[j % 3]
        for j, cell in enumerate(cells[k:]):
            yf[cell] = vals[j % 3]
        x = xf.reshape(G, C, H, W, M).transpose(0, 4, 1, 2, 3)
        for slot in range(2):                                  # a few NaN climatology cells in the anomaly's channel
            for cell in rng.permutation(H * W)[:max(1, H * W // 200)]:
                clim[slot, 3].reshape(-1)[cell] = np.nan
    x = np.ascontiguousarray(x, f32).reshape(G * M, C, H, W)
    idx = np.array([(g + 1) % 2 for g in range(G)], np.int32)
    return x, np.ascontiguousarray(y), clim, idx


def make_sources(truth, clim, idx):
    """(the ``events`` dict of the table, the oracle's source list): thresholds at the quantiles of the truth's values"""
    events, sources = {}, []
    G, _, H, W = truth.shape
    for label, (source, kind, c0, c1, direction, qs, _) in SOURCES.items():
        src = {"kind": kind, "c0": c0, "c1": c1, "direction": direction, "thresholds": []}
        rows_ = PO.clim_planes(src, clim, idx, G, H, W)
        x, valid = PO.source_value(truth, kind, c0, c1, rows_)
        if rows_ is not None:
            valid = valid & np.isfinite(rows_)
        src["thresholds"] = PO.quantile_thresholds(x, valid, direction, qs)
        events[label] = {"source": source, "thresholds": list(src["thresholds"]), "direction": direction}
        sources.append(src)
    return events, sources


def check_design(case, fc, truth, clim, idx, M, sources, band_w, bins=True):
    """the oracle on the inputs, before they are relied on; returns (acc, report64)"""
    acc, detail = PO.joint_rows(fc, truth, M, sources, clim, idx)
    nV, joint = PO.split(acc, M)
    for (label, spec), src, (valid, o, k, _), s in zip(SOURCES.items(), sources, detail, range(len(sources))):
        invalid = 1.0 - valid.mean()
        nt = len(src["thresholds"])
        assert (joint[s, :, :nt].sum(axis=(-1, -2)) == nV[s][:, None]).all() and (joint[s, :, nt:] == 0).all()
        if not bins:
            continue
        cells = valid.size
        assert cells >= (2340 if M == 32 else 640), (case, label, "cells", cells)
        assert 0.01 <= invalid <= 0.10, (case, label, "invalid fraction", invalid)
        for j in range(nt):
            yes = int(o[j][valid].sum())
            assert 0 < yes < int(valid.sum()), (case, label, j, "no truth event or no non-event")
        median = joint[s, :, spec[6]].sum(axis=0)                          # [2, M + 1]
        assert (median > 0).all(), (case, label, "an empty bin at the median threshold", median.tolist())
        print(f"PROB | {case} | {label} | cells {cells} | invalid {invalid:.3f} | smallest median bin "
              f"{int(median.min())}")
    rep = PO.report(acc, band_w, M, [len(s["thresholds"]) for s in sources])
    return acc, rep


def place(fc, truth, M, layout):
    """device tensors holding ``fc`` / ``truth`` in the memory layout of the case"""
    B, _, H, W = fc.shape
    f, t = torch.from_numpy(fc), torch.from_numpy(truth)
    if layout == "dense":
        return f.cuda(), t.cuda()
    if layout == "offset":                                     # one float off alignment: the scalar path
        v = torch.zeros(f.numel() + 1, device="cuda")[1:].view(B, C, H, W)
        v.copy_(f)
        assert v.data_ptr() % 16 == 4
        return v, t.cuda()
    chunk = torch.full((B, 3, C, H, W), float("nan"), device="cuda")        # "views": chunk[:, slot], truth[::M, k]
    true = torch.full((B, 2, C, H, W), float("nan"), device="cuda")
    chunk[:, 1] = f.cuda()
    true[::M, 1] = t.cuda()
    fv, tv = chunk[:, 1], true[::M, 1]
    assert fv.stride(0) == 3 * C * H * W and (tv.shape[0] == 1 or tv.stride(0) == 2 * M * C * H * W)
    return fv, tv


def fresh(H, M, events, clim, n_leads=2):
    from paradis_model_amd.probability import ProbabilityTable
    return ProbabilityTable(NAMES, lat_deg(H), n_leads, events, M, bands=BANDS,
                            climatology=torch.from_numpy(clim).cuda())


def judge(J, table, lead, acc, rep64, n_samples, values=True):
    """one lead of a table against the oracle's accumulators and report"""
    from paradis_model_amd.probability import CURVES, SCORES
    got = table.acc[lead].cpu().numpy()
    assert got.dtype == np.int64 and got.shape == acc.shape
    assert np.array_equal(got, acc), ("accumulator", np.argwhere(got != acc)[:5].tolist())
    assert table.n_samples.tolist() == n_samples
    cnt = table.counts()
    nV, joint = PO.split(acc, table.members)
    assert np.array_equal(cnt["valid"][lead], nV) and cnt["n_samples"].tolist() == n_samples
    for s, nt in enumerate(table.n_thresholds):
        assert np.array_equal(cnt["joint"][lead, s, :, :nt], joint[s, :, :nt])
        assert (cnt["joint"][lead, s, :, :nt].sum(axis=(-1, -2)) == cnt["valid"][lead, s][:, None]).all()
    if not values:
        return None
    res = table.result()
    for m in SCORES + CURVES:
        ref, mine = rep64[m], res[m][lead]
        assert mine.shape == ref.shape and np.array_equal(np.isnan(mine), np.isnan(ref)), m
        live = ~np.isnan(ref)
        scale = np.where(ref[live] != 0, np.abs(ref[live]), 1.0)
        J.add(m, float((np.abs(mine[live] - ref[live]) / scale).max()), FWD)
    ident = res["reliability"][lead] - res["resolution"][lead] + res["uncertainty"][lead]
    live = ~np.isnan(res["brier"][lead])
    J.add("brier - (rel - res + unc)", float(np.abs(res["brier"][lead] - ident)[live].max()), 1e-12)
    return res


# ================================================================================================ 1. the kernel pair
# name -> (G, M, H, W, layout[, seed]); M = 0: the library's maximum; H = 0: 2 rows(W) + 1, three row groups; the seed
# is 900 + the case's position where the oracle accepts that design (check_design), else one it accepts
CASES = {
    "M=2 G=3 64x5":                    (3, 2, 5, 64, "dense"),
    "M=3 G=1 260x9":                   (1, 3, 9, 260, "dense"),
    "M=4 G=1 1440 three groups":       (1, 4, 0, 1440, "dense"),
    "M=5 G=3 64x5 views":              (3, 5, 5, 64, "views"),
    "M=16 G=3 260x9":                  (3, 16, 9, 260, "dense"),
    "M=17 G=3 64x5":                   (3, 17, 5, 64, "dense"),
    "M=max G=1 260x9":                 (1, 0, 9, 260, "dense", 916),
    "M=max G=1 1440 three groups":     (1, 0, 0, 1440, "views"),
    "M=2 G=3 66x5 scalar":             (3, 2, 5, 66, "dense"),
    "M=3 G=3 66x5 scalar":             (3, 3, 5, 66, "dense"),
    "M=4 G=3 64x5 offset (scalar)":    (3, 4, 5, 64, "offset"),
    "M=5 G=3 66x5 scalar views":       (3, 5, 5, 66, "views"),
    "M=16 G=1 260x9 offset (scalar)":  (1, 16, 9, 260, "offset"),
    "M=17 G=3 66x5 scalar":            (3, 17, 5, 66, "dense"),
    "M=max G=3 66x12 scalar":          (3, 0, 12, 66, "dense"),
    "M=max G=1 260x9 offset (scalar)": (1, 0, 9, 260, "offset", 925),
    # the remainders 6 and 7 of the 8-deep member pipeline of the plain and anomaly sources
    "M=7 G=3 64x5":                    (3, 7, 5, 64, "dense"),
    "M=14 G=1 260x9":                  (1, 14, 9, 260, "dense"),
    "M=7 G=3 66x5 scalar":             (3, 7, 5, 66, "dense"),
    "M=14 G=3 66x5 scalar":            (3, 14, 5, 66, "dense"),
}
TINY = {"M=3 G=1 3x2": (1, 3, 2, 3), "M=2 G=3 1x1": (3, 2, 1, 1), "M=max G=3 3x2": (3, 0, 2, 3)}


def resolve(spec):
    G, M, H, W = spec[:4]
    return G, M or mmax(), H or 2 * rows(W) + 1, W


@pytest.mark.parametrize("case", list(CASES))
def test_update_at_dispatch_edges(case, record_property):
    G, M, H, W = resolve(CASES[case])
    layout = CASES[case][4]
    assert mmax() == 32 and rows(W) >= 1
    seed = CASES[case][5] if len(CASES[case]) > 5 else 900 + list(CASES).index(case)
    fc, truth, clim, idx = design(seed, G, M, H, W)
    events, sources = make_sources(truth, clim, idx)
    table = fresh(H, M, events, clim)
    assert table.T == 8 and table.acc.shape == (2, 4, H, 1 + 8 * 2 * (M + 1))
    acc, rep64 = check_design(case, fc, truth, clim, idx, M, sources, table.band_w)
    f, t = place(fc, truth, M, layout)
    before = (f.clone(), t.clone())
    table.update(1, f, t, torch.from_numpy(idx).cuda())
    assert torch.equal(f.nan_to_num(7.0), before[0].nan_to_num(7.0)) and \
        torch.equal(t.nan_to_num(7.0), before[1].nan_to_num(7.0))              # neither input is written
    J = _Judge(record_property, case)
    res = judge(J, table, 1, acc, rep64, [0, G])
    J.done()
    assert res["count"].tolist() == [0, G] and res["members"] == M and res["bands"] == list(BANDS)
    assert res["labels"] == list(SOURCES) and res["directions"] == ["ge", "ge", "ge", "le"]
    from paradis_model_amd.probability import CURVES, SCORES
    assert all(np.isnan(res[m][0]).all() for m in SCORES + CURVES)             # the lead never updated
    assert int(table.acc[0].abs().sum()) == 0
    seen = G * W * table.band_w.sum(axis=1)
    assert np.abs(res["valid_fraction"][1] - rep64["valid"] / seen[None, :]).max() <= 1e-12


@pytest.mark.parametrize("case", list(TINY))
def test_update_on_tiny_grids(case, record_property):
    """3 x 2 and 1 x 1: fewer cells than a quad's lanes; the integers alone"""
    G, M, H, W = resolve(TINY[case])
    fc, truth, clim, idx = design(950 + list(TINY).index(case), G, M, H, W, bad=H * W > 1)
    events, sources = make_sources(truth, clim, idx)
    table = fresh(H, M, events, clim)
    acc, _ = check_design(case, fc, truth, clim, idx, M, sources, table.band_w, bins=False)
    table.update(0, torch.from_numpy(fc).cuda(), torch.from_numpy(truth).cuda(), torch.from_numpy(idx).cuda())
    judge(_Judge(record_property, case), table, 0, acc, None, [G, 0], values=False)


# ================================================================================================ 2. bit-level promises
def _equal(a, b):
    return torch.equal(a.acc, b.acc) and torch.equal(a.n_samples, b.n_samples)


@pytest.mark.parametrize("M", [5, 0])
def test_bit_level_promises(M, record_property):
    M = M or mmax()
    G, W, H = 3, 260, 9
    fc, truth, clim, idx = design(700 + M, G, M, H, W)
    events, sources = make_sources(truth, clim, idx)
    new = lambda: fresh(H, M, events, clim)                                    # noqa: E731
    kd = torch.from_numpy(idx).cuda()
    fv, tv = place(fc, truth, M, "dense")
    fs, ts = place(fc, truth, M, "offset")
    a, b, c = new(), new(), new()
    a.update(0, fv, tv, kd)
    b.update(0, fs, ts, kd)
    c.update(0, fv, tv, kd)
    assert _equal(a, b), "the scalar path and the vector path differ"
    assert _equal(a, c), "two runs differ"
    acc, rep64 = check_design(f"promises M={M}", fc, truth, clim, idx, M, sources, a.band_w)
    J = _Judge(record_property, f"promises M={M}")
    judge(J, a, 0, acc, rep64, [G, 0])
    J.done()
    # updates of 1 and 2 ensembles == one update of the 3 concatenated
    two = new()
    two.update(0, fv[:M], tv[:1], kd[:1])
    assert two.n_samples.tolist() == [1, 0]
    two.update(0, fv[M:], tv[1:], kd[1:])
    assert _equal(two, a)
    # G == 0 leaves everything untouched
    keep = two.acc.clone()
    two.update(0, fv[:0], tv[:0], kd[:0])
    assert torch.equal(two.acc, keep) and two.n_samples.tolist() == [G, 0]
    # reset() clears
    two.reset()
    assert int(two.acc.abs().sum()) == 0 and int(two.n_samples.sum()) == 0
    assert np.isnan(two.result()["brier"]).all()
    two.update(0, fv, tv, kd)
    assert _equal(two, a)
    # batch-strided chunk[:, slot] / truth[::M, k] == dense copies
    fw, tw = place(fc, truth, M, "views")
    d = new()
    d.update(0, fw, tw, kd)
    assert _equal(d, a)
    # an ensemble whose clim_index is out of range adds nothing to the anomaly source and all of its cells to the others
    out = new()
    far = torch.tensor([int(idx[0]), 2, -1], dtype=torch.int32, device="cuda")
    out.update(0, fv, tv, far)
    first = new()
    first.update(0, fv[:M], tv[:1], kd[:1])
    s = list(SOURCES).index("anom")
    others = [i for i in range(len(SOURCES)) if i != s]
    assert torch.equal(out.acc[0, s], first.acc[0, s]) and torch.equal(out.acc[0, others], a.acc[0, others])
    assert out.n_samples.tolist() == [G, 0]
    want, _ = PO.joint_rows(fc, truth, M, sources, clim, [int(idx[0]), 2, -1])
    assert np.array_equal(out.acc[0].cpu().numpy(), want)


def test_update_is_graph_capturable():
    """an update captured in a HIP graph and replayed twice equals two eager updates"""
    from paradis_model_amd.harness import capture_forward
    G, M, H, W = 2, 4, 8, 64
    fc, truth, clim, idx = design(29, G, M, H, W)
    events, _ = make_sources(truth, clim, idx)
    fd, td, kd = torch.from_numpy(fc).cuda(), torch.from_numpy(truth).cuda(), torch.from_numpy(idx).cuda()
    eager = fresh(H, M, events, clim)
    eager.update(1, fd, td, kd)
    eager.update(1, fd, td, kd)
    graphed = fresh(H, M, events, clim)
    graph, _ = capture_forward(lambda: graphed.update(1, fd, td, kd), warmup=1)
    torch.cuda.synchronize()
    graphed.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(graphed, eager) and graphed.n_samples.tolist() == [0, 2 * G]
    assert int(eager.acc[1, :, :, 0].sum()) > 0


def test_update_refusals_on_the_device():
    from paradis_model_amd.probability import ProbabilityTable
    H, W, M = 4, 8, 2
    ev = {"warm": {"source": "c0", "thresholds": [0.0]}}
    table = ProbabilityTable(NAMES, lat_deg(H), 1, ev, M)
    x, y = torch.zeros(4, C, H, W, device="cuda"), torch.zeros(2, C, H, W, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        table.update(0, x.cpu(), y)
    with pytest.raises(ValueError, match="dense"):
        table.update(0, torch.zeros(4, C, H, 2 * W, device="cuda")[..., ::2], y)
    with pytest.raises(ValueError, match="whole ensembles"):
        table.update(0, x[:3], y)
    clim = torch.zeros(2, C, H, W, device="cuda")
    with_clim = ProbabilityTable(NAMES, lat_deg(H), 1, ev, M, climatology=clim)
    with pytest.raises(ValueError, match="must live on the device"):
        with_clim.update(0, x, y, torch.zeros(2, dtype=torch.int32))
    cpu_table = ProbabilityTable(NAMES, lat_deg(H), 1, ev, M, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu_table.update(0, x, y)
    assert int(table.acc.abs().sum()) == 0
    table.update(0, x, y)                                      # zeros: every cell valid, the event 0 >= 0 everywhere
    cnt = table.counts()
    assert (cnt["valid"] == 2 * W).all() and (cnt["joint"][0, 0, :, 0, 1, M] == 2 * W).all()
    assert int(cnt["joint"].sum()) == 2 * W * H


# ================================================================================================ 3. cross-checks
def test_identical_members_give_the_event_tables_counts():
    """all M members equal one forecast f: the four corner bins joint[j][o][0 or M] are EventTable's correct negatives /
    misses / false alarms / hits of f against the truth, bit for bit; every other bin is 0"""
    from paradis_model_amd.events import EventTable
    G, M, H, W = 3, 5, 9, 260
    fc, truth, clim, idx = design(41, G, M, H, W)
    f = np.ascontiguousarray(fc[::M])                          # member 0 of every ensemble (with its bad cells)
    events, _ = make_sources(truth, clim, idx)
    fd, td, kd = torch.from_numpy(f).cuda(), torch.from_numpy(truth).cuda(), torch.from_numpy(idx).cuda()
    table = fresh(H, M, events, clim, n_leads=1)
    table.update(0, fd.repeat_interleave(M, dim=0), td, kd)
    ev = EventTable(NAMES, lat_deg(H), 1, events, bands=BANDS, climatology=torch.from_numpy(clim).cuda())
    ev.update(0, fd, td, kd)
    cnt, ref = table.counts(), ev.counts()
    nV, nF, nO, nFO = (ref[k][0] for k in ("valid", "forecast_yes", "observed_yes", "both"))
    assert np.array_equal(cnt["valid"][0], nV) and int(nV.sum()) > 0
    joint = cnt["joint"][0]                                    # [S, H, T, 2, M + 1]
    for s, nt in enumerate(table.n_thresholds):
        j = slice(0, nt)
        assert np.array_equal(joint[s, :, j, 0, 0], (nV[s][:, None] - nF[s] - nO[s] + nFO[s])[:, j]), "correct negatives"
        assert np.array_equal(joint[s, :, j, 1, 0], (nO[s] - nFO[s])[:, j]), "misses"
        assert np.array_equal(joint[s, :, j, 0, M], (nF[s] - nFO[s])[:, j]), "false alarms"
        assert np.array_equal(joint[s, :, j, 1, M], nFO[s][:, j]), "hits"
        assert int(joint[s, :, j, :, 1:M].sum()) == 0
        assert int(joint[s, :, j, 1, M].sum()) > 0 and int(joint[s, :, j, 0, 0].sum()) > 0


def test_member_events_sum_to_the_event_tables_forecast_counts():
    """on a design without bad cells, sum_k k N_k equals the sum over the members of EventTable's forecast-event counts
    (and sum_k N_1k its observed-event counts)"""
    from paradis_model_amd.events import EventTable
    G, M, H, W = 2, 4, 5, 260
    fc, truth, clim, idx = design(43, G, M, H, W, bad=False)
    events, _ = make_sources(truth, clim, idx)
    fd, td, kd = torch.from_numpy(fc).cuda(), torch.from_numpy(truth).cuda(), torch.from_numpy(idx).cuda()
    table = fresh(H, M, events, clim, n_leads=1)
    table.update(0, fd, td, kd)
    ev = EventTable(NAMES, lat_deg(H), 1, events, bands=BANDS, climatology=torch.from_numpy(clim).cuda())
    for i in range(M):
        ev.update(0, fd[i::M], td, kd)                         # member i of every ensemble, in place
    cnt, ref = table.counts(), ev.counts()
    assert (cnt["valid"][0] == G * W).all() and (ref["valid"][0] == M * G * W).all()
    k = np.arange(M + 1)
    for s, nt in enumerate(table.n_thresholds):
        joint = cnt["joint"][0, s, :, :nt]                      # [H, nt, 2, M + 1]
        assert np.array_equal((joint.sum(axis=2) * k).sum(axis=-1), ref["forecast_yes"][0, s, :, :nt])
        assert np.array_equal(M * joint[:, :, 1].sum(axis=-1), ref["observed_yes"][0, s, :, :nt])


# ================================================================================================ 4. the forecaster hook
def test_forecaster_hook():
    """run(probability=table, ...) beside an ensemble card and a scorecard at 32x64 with B = 4, M = 2: the table equals
    ``table.update`` called by hand on the stored chunk with the truth and the climatology slot of each ensemble's first
    member; the card's and the scorecard's numbers are those of a run without the table; and the table alone"""
    from paradis_model_amd.ensemble import EnsembleCard
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.probability import ProbabilityTable
    from paradis_model_amd.verify import Scorecard
    from tests import forecast_oracle as FO
    from tests.test_hip_ens import _rollout_setup
    from tests.test_hip_verify import _Collect, lat_weights
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    Cn, M, K = spec.num_channels, 2, 3
    norm = FO.normalised_state(31, spec.names, B, S, Cn, H, W).cuda()
    phys = torch.empty(B, S, Cn, H, W, device="cuda")
    for s in range(S):
        postprocess(norm[:, s], spec, lat, lon, phys, s)
    a, b, c = spec.names[0], spec.names[5], spec.names[-1]
    med = lambda n: float(phys[:, :, spec.names.index(n)].median())           # noqa: E731
    clim = (phys[:K, 0] * 0.5).contiguous()
    events = {"plain": {"source": a, "thresholds": [med(a)]},
              "anom": {"source": ("anomaly", b), "thresholds": [0.5 * med(b), 0.0], "direction": "le"},
              "speed": {"source": ("speed", a, c), "thresholds": [abs(med(a)) + abs(med(c))]}}
    idx = torch.tensor([[0, 1], [2, 2], [2, 0], [1, 1]], dtype=torch.int32, device="cuda")       # [B, S]

    def new():
        return ProbabilityTable(spec.names, lat, S, events, M, bands=BANDS, climatology=clim)

    new_card = lambda: EnsembleCard(spec.names, lat, S, M, channels=[a, c], seed=2)             # noqa: E731
    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=True)
    new_score = lambda: Scorecard(spec.names, lat_weights(H), S, climatology=clim)                 # noqa: E731
    table, card, score = new(), new_card(), new_score()
    seen = _Collect()
    fc.run(*inputs, seen, probability=table, ensemble=card, scorecard=score, truth=phys, clim_index=idx)
    states = torch.cat([ch[1] for ch in seen.chunks], dim=1)                   # [B, S, C, H, W] as the writer saw them
    by_hand = new()
    for s in range(S):
        by_hand.update(s, states[:, s].cuda(), phys[::M, s], idx[::M, s].contiguous())
    assert _equal(table, by_hand) and table.n_samples.tolist() == [B // M] * S
    cnt = table.counts()
    assert (cnt["valid"] == (B // M) * W).all()
    res = table.result()
    assert np.isfinite(res["brier"][:, 0, :, 0]).all() and np.isfinite(res["valid_fraction"]).all()
    without_score, without_card = new_score(), new_card()
    fc.run(*inputs, None, ensemble=without_card, scorecard=without_score, truth=phys, clim_index=idx)
    assert torch.equal(score.acc, without_score.acc)
    assert torch.equal(card.acc_real, without_card.acc_real) and torch.equal(card.acc_int, without_card.acc_int)
    only = new()
    fc.run(*inputs, None, probability=only, truth=phys, clim_index=idx)        # without the other tables
    assert _equal(only, table)
    with pytest.raises(ValueError, match="probability table has 3 members"):
        fc.run(*inputs, None, probability=ProbabilityTable(spec.names, lat, S, events, 3, climatology=clim), truth=phys,
               clim_index=idx)
    with pytest.raises(ValueError, match="probability table needs truth"):
        fc.run(*inputs, None, probability=table)
    with pytest.raises(ValueError, match="leads"):
        fc.run(*inputs, None, probability=ProbabilityTable(spec.names, lat, S - 1, events, M, climatology=clim),
               truth=phys, clim_index=idx)
    assert _equal(table, by_hand)
