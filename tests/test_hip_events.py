"""Event verification on the device (csrc/events.hip) against the numpy restatement tests/events_oracle.py - EXACTLY:
the decision is discrete and the counts are integers, so ``counts()`` must equal the oracle's arrays bit for bit
(``np.array_equal``), whichever load path, row group or threshold variant produced them; ``result()`` applies float64
weights to those integers and agrees with the oracle's row-by-row sums within 1e-12 (non-negative terms: any order is
within (H + 1) 2^-53 of exact).

Every design first goes through the oracle on the CPU, which must report (``judge_design``) zero ambiguous cells -
cells within 4 fp32 ulps of a threshold that are not exact ties, where another correct evaluation could decide the
other way; the planted exact ties are the only cells at a threshold - and, in every row of every source, for at least
one threshold non-zero ``nFO``, ``nF - nFO`` and ``nO - nFO``: a dropped or doubled cell in any row changes an integer.

Designs: standard-normal truth, forecast = truth + 0.6 noise + 0.1, thresholds at about the 0.3 / 0.6 / 0.9 quantiles
of each source (all exactly representable); the first cell of every row is planted beyond the highest threshold in the
forecast and below the lowest in the truth, the last cell the other way round; cells 1 and 2 of row 0 of sample 0 hold
exact ties in forecast and truth (plain: the value is the threshold; anomaly: 1.0 - 0.75 = 0.25; speed: 3-4-5).
Shapes come from ``paradis_events_rows(W)``."""
import numpy as np
import pytest
import torch

from paradis_model_amd import _lib
from paradis_model_amd import events as EV
from tests import events_oracle as EO

pytestmark = pytest.mark.gpu

NAMES = ["tp", "u10", "v10", "t2m"]                  # channel 0 plain, 1 / 2 the speed's components, 3 the anomaly's
THR = {"plain": [-0.5, 0.25, 1.25], "speed": [0.875, 5.0, 2.125, 1.375], "anomaly": [-0.5, 0.25, 1.5]}
THR8 = [1.25, -0.5, 0.25, 2.0, -1.0, 0.75, -1.5, 0.0]                     # unsorted
BANDS = {"global": (-90.0, 90.0), "nh": (0.0, 90.0)}


def rows(W):
    return int(_lib.lib.paradis_events_rows(W))


def lat_deg(H):
    return np.linspace(-88.0, 88.0, H) if H > 1 else np.zeros(1)


def make_sources(kinds, thr=None, direction="ge"):
    """(events dict of EventTable, source list of the oracle)"""
    ev, srcs = {}, []
    for kind in kinds:
        t = list(THR[kind] if thr is None else thr)
        if kind == "plain":
            ev["rain"] = {"source": "tp", "thresholds": t, "direction": direction}
            srcs.append({"kind": "plain", "c0": 0, "thresholds": t, "direction": direction})
        elif kind == "speed":
            ev["gale"] = {"source": ("speed", "u10", "v10"), "thresholds": t, "direction": direction}
            srcs.append({"kind": "speed", "c0": 1, "c1": 2, "thresholds": t, "direction": direction})
        else:
            ev["warm"] = {"source": ("anomaly", "t2m"), "thresholds": t, "direction": direction}
            srcs.append({"kind": "anomaly", "c0": 3, "thresholds": t, "direction": direction})
    return ev, srcs


def design(seed, B, H, W, K=1):
    """(forecast, truth [B, 4, H, W], clim [K, 4, H, W]) float32 numpy, planted as the module docstring says"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((B, 4, H, W)).astype(np.float32)
    f = (t + np.float32(0.6) * rng.standard_normal((B, 4, H, W)).astype(np.float32) + np.float32(0.1)).astype(np.float32)
    clim = (np.float32(0.5) * rng.standard_normal((K, 4, H, W)).astype(np.float32)).astype(np.float32)
    clim[..., 0] = clim[..., W - 1] = 0.0
    for x, y, col in ((f, t, 0), (t, f, W - 1)):        # x beyond every threshold, y below every one
        x[:, 0, :, col], y[:, 0, :, col] = 3.0, -3.0
        x[:, 1, :, col] = x[:, 2, :, col] = 4.0
        y[:, 1, :, col] = y[:, 2, :, col] = 0.125
        x[:, 3, :, col], y[:, 3, :, col] = 5.0, -5.0
    if W >= 4:                                           # exact ties: cell 1 in the forecast, cell 2 in the truth
        for x, col in ((f, 1), (t, 2)):
            x[0, 0, 0, col] = 0.25
            x[0, 1, 0, col], x[0, 2, 0, col] = 3.0, 4.0
            x[0, 3, 0, col] = 1.0
        clim[:, 3, 0, 1:3] = 0.75
    return f, t, clim


def judge_design(cnt, srcs):
    """the oracle's verdict on a design: one answer only, and every row can show a lost or doubled cell"""
    assert cnt["ambiguous"] == 0
    for s, src in enumerate(srcs):
        n = len(src["thresholds"])
        nF, nO, nFO = (cnt[k][s, :, :n] for k in ("forecast_yes", "observed_yes", "both"))
        live = ((nFO > 0) & (nF - nFO > 0) & (nO - nFO > 0)).any(axis=1)
        assert live.all(), (s, np.flatnonzero(~live))
        assert (cnt["valid"][s] > 0).all()


def fill_expected(table, per_lead):
    """the oracle's counts dict per lead -> arrays shaped like ``EventTable.counts()``"""
    L, S, H, T = table.n_leads, len(table.labels), table.H, table.T
    want = {"valid": np.zeros((L, S, H), np.int64), "n_samples": np.zeros(L, np.int64)}
    for k in ("forecast_yes", "observed_yes", "both"):
        want[k] = np.zeros((L, S, H, T), np.int64)
        for s, n in enumerate(table.n_thresholds):
            want[k][:, s, :, n:] = -1
    for lead, (cnt, B) in per_lead.items():
        want["valid"][lead] = cnt["valid"]
        want["n_samples"][lead] = B
        for k in ("forecast_yes", "observed_yes", "both"):
            want[k][lead] = np.where(cnt[k] < 0, -1, cnt[k])
    return want


def assert_counts(table, per_lead):
    got = table.counts()
    want = fill_expected(table, per_lead)
    for k in ("n_samples", "valid", "forecast_yes", "observed_yes", "both"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), \
            (k, np.argwhere(got[k] != want[k])[:5].tolist())
    res = table.result()
    again = EV.scores(*(res[k] for k in EV.TABLES))
    for k in EV.SCORES:
        assert np.array_equal(res[k], again[k], equal_nan=True), k
    for lead, (cnt, B) in per_lead.items():
        for k, ref in zip(EV.TABLES, EO.tables(cnt, table.band_w)):
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(res[k][lead]), ~fin), k
            assert np.all(np.abs(res[k][lead][fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin])), k
    return res


def run_design(f, t, clim, kidx, ev, srcs, H, n_leads=2, lead=0, place=None):
    """oracle first, then one update on the device; returns (table, oracle counts)"""
    B = f.shape[0]
    with_clim = any(s["kind"] == "anomaly" for s in srcs)
    cnt = EO.counts(f, t, srcs, clim if with_clim else None, kidx)
    judge_design(cnt, srcs)
    climd = torch.from_numpy(clim).cuda() if with_clim else None
    table = EV.EventTable(NAMES, lat_deg(H), n_leads, ev, bands=BANDS, climatology=climd)
    fd, td = (place or (lambda x: torch.from_numpy(x).cuda()))(f), torch.from_numpy(t).cuda()
    kd = None if (kidx is None or not with_clim) else torch.from_numpy(np.asarray(kidx, np.int32)).cuda()
    table.update(lead, fd, td, kd)
    assert_counts(table, {lead: (cnt, B)})
    return table, cnt


# ================================================================================================ 1. grids
def _grid_cases():
    R = rows(64)
    return [("headline 32x64", 2, 32, 64), ("a workgroup that owns one row", 1, R + 1, 64), ("one row", 3, 1, 64),
            ("W below a wave's quads", 3, 3, 4), ("W % 4 != 0", 3, 5, 6), ("4x68: one quad into a second wave-width", 2, 4, 68),
            ("4x260: one quad into a second walk", 2, 4, 260), ("crosses a row group of 5", 1, 6, 1440), ("a long row on the scalar path", 2, 2, 1030)]


@pytest.mark.parametrize("case", _grid_cases(), ids=lambda c: c[0])
def test_counts_at_grid_edges(case):
    """all three source kinds in one launch at every grid edge (4x68: a row that ends one quad past 64 cells; 4x260: a
    row that ends one quad into the second 256-cell walk of a wave)"""
    _, B, H, W = case
    assert rows(1440) == 5 and rows(64) == 128
    f, t, clim = design(100 + H + W, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    run_design(f, t, clim, None, ev, srcs, H)


# ================================================================================================ 2. sources, thresholds
SOURCE_CASES = [("plain", ("plain",), None, "ge"), ("speed", ("speed",), None, "ge"), ("anomaly", ("anomaly",), None, "ge"),
                ("all three", ("plain", "speed", "anomaly"), None, "ge"), ("T=1", ("plain",), [0.25], "ge"),
                ("T=2", ("plain", "anomaly"), [0.25, -0.5], "ge"), ("T=8 unsorted", ("plain", "anomaly"), THR8, "ge"),
                ("le", ("plain", "speed", "anomaly"), None, "le"),
                # (thresholds rounded up to a compiled variant: 3 -> 4 and 5 -> 8, the rest padded with NaN)
                ("T=3", ("plain", "speed"), [0.25, -0.5, 1.0], "ge"), ("T=5", ("plain", "anomaly"), THR8[:5], "le")]


@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
@pytest.mark.parametrize("case", SOURCE_CASES, ids=lambda c: c[0])
def test_sources_and_thresholds(case, H, W):
    _, kinds, thr, direction = case
    B = 2
    f, t, clim = design(7, B, H, W, K=2)
    ev, srcs = make_sources(kinds, thr, direction)
    table, _ = run_design(f, t, clim, np.array([1, 0]), ev, srcs, H)
    assert table.T == max(len(s["thresholds"]) for s in srcs)


@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
def test_mixed_and_out_of_range_climatology_slots(H, W):
    """K = 2 with mixed clim_index and one slot out of range: that sample adds nothing to the anomaly source (and
    nothing of it is read), the other sources do not notice"""
    B = 3
    f, t, clim = design(11, B, H, W, K=2)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    table, cnt = run_design(f, t, clim, np.array([1, 2, 0]), ev, srcs, H)
    assert (cnt["valid"][2] == 2 * W).all() and (cnt["valid"][0] == 3 * W).all()
    inside = EO.counts(f[[0, 2]], t[[0, 2]], srcs, clim, np.array([1, 0]))
    for k in ("valid", "forecast_yes", "observed_yes", "both"):
        assert np.array_equal(cnt[k][2], inside[k][2]), k
    below = EV.EventTable(NAMES, lat_deg(H), 1, ev, climatology=torch.from_numpy(clim).cuda())
    below.update(0, torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda(), torch.tensor([1, -1, 0], dtype=torch.int32).cuda())
    assert torch.equal(below.acc[0], table.acc[0])


@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_cells_leave_every_class(bad, H, W):
    """NaN / +-Inf in the forecast only, the truth only, the speed's second component only and the climatology only
    each remove exactly that cell from every class of the sources that read it"""
    B = 2
    f, t, clim = design(31, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    base = EO.counts(f, t, srcs, clim, None)
    h, w = H // 2, W // 2 + 1
    f[0, 0, h, w] = bad             # plain: forecast only
    t[1, 0, h, w + 1] = bad         # plain: truth only
    f[1, 2, h, w] = bad             # speed: second component, forecast only
    t[0, 1, h, w + 2] = bad         # speed: first component, truth only
    f[0, 3, h, w] = bad             # anomaly: forecast only
    clim[0, 3, h, w + 3] = bad      # anomaly: climatology only (both samples read slot 0)
    clim[0, 0, h, w + 4] = bad      # a climatology plane that no source reads
    _, cnt = run_design(f, t, clim, None, ev, srcs, H)
    gone = base["valid"] - cnt["valid"]
    want = np.zeros_like(gone)
    want[:, h] = (2, 2, 3)
    assert np.array_equal(gone, want)


# ================================================================================================ 3. layouts
@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
def test_offset_forecast_takes_the_scalar_path_and_equals_dense(H, W):
    B = 2
    f, t, clim = design(17, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    dense, _ = run_design(f, t, clim, None, ev, srcs, H)

    def offset(x):
        buf = torch.zeros(x.size + 1, device="cuda")
        view = buf[1:].view(*x.shape)
        view.copy_(torch.from_numpy(x))
        assert view.data_ptr() % 16 == 4
        return view

    shifted, _ = run_design(f, t, clim, None, ev, srcs, H, place=offset)
    assert torch.equal(shifted.acc, dense.acc) and torch.equal(shifted.n_samples, dense.n_samples)


def test_views_of_a_chunk_and_a_stored_truth():
    B, H, W = 2, 32, 64
    f, t, clim = design(19, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    dense, cnt = run_design(f, t, clim, None, ev, srcs, H)
    chunk = torch.full((B, 3, 4, H, W), float("nan"), device="cuda")
    true = torch.full((B, 3, 4, H, W), float("nan"), device="cuda")
    chunk[:, 1], true[:, 1] = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    table = EV.EventTable(NAMES, lat_deg(H), 2, ev, bands=BANDS, climatology=torch.from_numpy(clim).cuda())
    table.update(0, chunk[:, 1], true[:, 1])
    assert torch.equal(table.acc, dense.acc)
    odd = torch.zeros(B, 4 * H * W + 1, device="cuda")[:, :4 * H * W].view(B, 4, H, W)     # a batch stride of 4 k + 1
    odd.copy_(torch.from_numpy(f))
    table.reset()
    table.update(0, odd, true[:, 1])
    assert torch.equal(table.acc, dense.acc)


# ================================================================================================ 4. invariants
def test_bit_level_promises():
    H, W = 6, 1440
    f, t, clim = design(23, 5, H, W, K=2)
    kidx = np.array([0, 1, 1, 0, 1])
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    cnt = EO.counts(f, t, srcs, clim, kidx)
    judge_design(cnt, srcs)
    fd, td, kd = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(kidx.astype(np.int32)).cuda()
    climd = torch.from_numpy(clim).cuda()

    def fresh():
        return EV.EventTable(NAMES, lat_deg(H), 3, ev, bands=BANDS, climatology=climd)

    a, b, c = fresh(), fresh(), fresh()
    a.update(1, fd, td, kd)
    b.update(1, fd, td, kd)
    assert torch.equal(a.acc, b.acc)                                       # run == run
    assert_counts(a, {1: (cnt, 5)})
    assert int(a.acc[0].abs().sum()) == 0 and int(a.acc[2].abs().sum()) == 0     # another lead's rows are untouched
    c.update(1, fd[:2], td[:2], kd[:2])
    c.update(1, fd[2:], td[2:], kd[2:])
    assert torch.equal(c.acc, a.acc) and c.n_samples.tolist() == [0, 5, 0]       # 2 + 3 == the concatenated 5
    a.update(1, fd[:0], td[:0], kd[:0])                                    # B == 0 returns
    assert torch.equal(c.acc, a.acc)
    d = fresh()
    d.acc[1].fill_(2 ** 32 - 1)
    d.n_samples[1] = 2 ** 32 - 1
    d.update(1, fd, td, kd)
    assert torch.equal(d.acc[1] - (2 ** 32 - 1), a.acc[1])                 # the carry into the upper word
    assert int(d.acc[1].max()) > 2 ** 32 and d.n_samples.tolist() == [0, 2 ** 32 + 4, 0]
    a.reset()
    assert int(a.acc.abs().sum()) == 0 and int(a.n_samples.sum()) == 0


def test_update_refusals_on_the_device():
    H, W = 4, 8
    ev, _ = make_sources(("plain",))
    table = EV.EventTable(NAMES, lat_deg(H), 1, ev)
    x = torch.zeros(2, 4, H, W, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        table.update(0, x.cpu(), x)
    with pytest.raises(ValueError, match="dense"):
        table.update(0, torch.zeros(2, 4, H, 2 * W, device="cuda")[..., ::2], x)
    cpu_table = EV.EventTable(NAMES, lat_deg(H), 1, ev, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu_table.update(0, x, x)
    assert int(table.acc.abs().sum()) == 0


# ================================================================================================ 5. integration
def test_update_is_graph_capturable():
    """an update captured in a HIP graph and replayed twice equals two eager updates"""
    from paradis_model_amd.harness import capture_forward
    B, H, W = 2, 32, 64
    f, t, clim = design(29, B, H, W, K=2)
    ev, _ = make_sources(("plain", "speed", "anomaly"))
    fd, td, climd = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(clim).cuda()
    kd = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    eager = EV.EventTable(NAMES, lat_deg(H), 2, ev, climatology=climd)
    eager.update(1, fd, td, kd)
    eager.update(1, fd, td, kd)
    graphed = EV.EventTable(NAMES, lat_deg(H), 2, ev, climatology=climd)
    graph, _ = capture_forward(lambda: graphed.update(1, fd, td, kd), warmup=1)
    torch.cuda.synchronize()
    graphed.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.acc, eager.acc) and graphed.n_samples.tolist() == [0, 2 * B]


@pytest.mark.parametrize("truth_normalized,graph,with_card", [(False, False, False), (True, True, True)])
def test_forecaster_hook(truth_normalized, graph, with_card):
    """run(events=..., truth=...) counts the chunks it hands to on_chunk: bit for bit the accumulators of a table updated
    by hand with those chunks; the chunks are those of a run without a table; beside a scorecard both get the same
    states and the same clim_index column"""
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.verify import Scorecard
    from tests import forecast_oracle as FO
    from tests.test_hip_verify import _Collect, _rollout_setup, lat_weights
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    C = spec.num_channels
    norm = FO.normalised_state(31, spec.names, B, S, C, H, W).cuda()
    phys = torch.empty(B, S, C, H, W, device="cuda")
    clim = torch.empty(1, 2, C, H, W, device="cuda")
    cnorm = FO.normalised_state(32, spec.names, 1, 2, C, H, W).cuda()
    for s in range(S):
        postprocess(norm[:, s], spec, lat, lon, phys, s)
    for s in range(2):
        postprocess(cnorm[:, s], spec, lat, lon, clim, s)
    clim = clim[0].contiguous()
    kidx = torch.tensor([[0, 1, 1], [1, 0, 1]], dtype=torch.int32, device="cuda")
    n0, n1, n2 = spec.names[0], spec.names[1], spec.names[-1]     # thresholds at the medians of the truth
    med = {n: float(phys[:, :, spec.names.index(n)].median()) for n in (n0, n2)}
    sp = torch.sqrt(phys[:, :, spec.names.index(n0)] ** 2 + phys[:, :, spec.names.index(n1)] ** 2)
    ev = {"a": {"source": n0, "thresholds": [med[n0]]},
          "s": {"source": ("speed", n0, n1), "thresholds": [float(sp.median()), float(sp.mean())], "direction": "le"},
          "w": {"source": ("anomaly", n2), "thresholds": [0.0]}}

    def fresh():
        return EV.EventTable(spec.names, lat, S, ev, bands={"sh": (-90.0, 0.0), "nh": (0.0, 90.0)}, climatology=clim)

    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=graph)
    plain = _Collect()
    fc.run(*inputs, plain)
    table = fresh()
    card = Scorecard(spec.names, lat_weights(H), S, climatology=clim) if with_card else None
    scored = _Collect()
    fc.run(*inputs, scored, events=table, scorecard=card, truth=norm if truth_normalized else phys,
           truth_normalized=truth_normalized, clim_index=kidx)
    assert [c[0] for c in scored.chunks] == [0, 2] and [c[1].shape[1] for c in scored.chunks] == [2, 1]
    for (s0, x), (s1, y) in zip(plain.chunks, scored.chunks):
        assert s0 == s1 and torch.equal(x, y)                               # the chunk contents are unchanged
    states = torch.cat([c[1] for c in scored.chunks], dim=1)
    by_hand = fresh()
    for s in range(S):
        by_hand.update(s, states[:, s].cuda(), phys[:, s], kidx[:, s].contiguous())
    assert torch.equal(table.acc, by_hand.acc) and torch.equal(table.n_samples, by_hand.n_samples)
    assert table.n_samples.tolist() == [B] * S
    cnt = table.counts()
    assert (cnt["valid"] == B * W).all() and (cnt["observed_yes"][:, 0, :, 0].sum() > 0)
    if with_card:
        alone = Scorecard(spec.names, lat_weights(H), S, climatology=clim)
        fc.run(*inputs, None, scorecard=alone, truth=norm if truth_normalized else phys,
               truth_normalized=truth_normalized, clim_index=kidx)
        assert torch.equal(card.acc, alone.acc)
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, events=table, truth=phys[:, :2])              # a wrong n_stored: before the rollout
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, events=table)
    with pytest.raises(ValueError, match="leads"):
        fc.run(*inputs, None, events=EV.EventTable(spec.names, lat, S - 1, ev, climatology=clim), truth=phys)
    assert torch.equal(table.acc, by_hand.acc)
