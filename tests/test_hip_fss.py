"""Neighbourhood verification on the device (csrc/fss.hip) against the numpy restatement tests/fss_oracle.py - EXACTLY:
the decision is discrete and everything after it is an integer, so ``FractionsTable.counts()`` must equal the oracle's
int64 arrays bit for bit (``np.array_equal``), whichever load path, workgroup, halo or threshold variant produced them.

Designs are those of tests/test_hip_events.py (standard-normal truth, forecast = truth + 0.6 noise + 0.1, planted cells
at both row ends, exact ties), which the events oracle judges first: zero ambiguous cells, every row live.  Shapes come
from ``paradis_fss_rows(W, ny_max)`` and the limit getters."""
import numpy as np
import pytest
import torch

from paradis_model_amd import _lib
from paradis_model_amd import events as EV
from paradis_model_amd import neighbourhood as NB
from tests import events_oracle as EO
from tests import fss_oracle as FO
from tests.test_hip_events import BANDS, NAMES, THR8, design, judge_design, lat_deg, make_sources

pytestmark = pytest.mark.gpu

L = _lib.lib
NY_MAX = int(L.paradis_fss_max_half_y())
K_MAX = int(L.paradis_fss_max_scales())


def rows(W, ny_max=NY_MAX):
    return int(L.paradis_fss_rows(W, ny_max))


def expected(table, per_lead):
    """the oracle's arrays per lead -> arrays shaped like ``FractionsTable.counts()``"""
    Ln, S, H, T, K = table.n_leads, len(table.labels), table.H, table.T, len(table.scales)
    want = {"valid": np.zeros((Ln, S, H), np.int64), "n_samples": np.zeros(Ln, np.int64)}
    for k, shape in (("forecast_yes", (Ln, S, H, T)), ("observed_yes", (Ln, S, H, T)), ("ff", (Ln, S, H, K, T)),
                     ("oo", (Ln, S, H, K, T)), ("fo", (Ln, S, H, K, T))):
        want[k] = np.zeros(shape, np.int64)
        for s, n in enumerate(table.n_thresholds):
            want[k][:, s, ..., n:] = -1
    for lead, (cnt, B) in per_lead.items():
        want["n_samples"][lead] = B
        for k in FO.KEYS:
            want[k][lead] = cnt[k]
    return want


def assert_counts(table, per_lead):
    got, want = table.counts(), expected(table, per_lead)
    for k in ("n_samples",) + FO.KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), \
            (k, np.argwhere(got[k] != want[k])[:5].tolist())


def to_dev(x):
    return torch.from_numpy(x).cuda()


def run_design(f, t, clim, kidx, ev, srcs, scales, n_leads=2, lead=0, place=None, judge=True, **table_kw):
    """the oracles first, then one update on the device; returns (table, oracle counts)"""
    B, _, H, W = f.shape
    with_clim = any(s["kind"] == "anomaly" for s in srcs)
    if judge:
        judge_design(EO.counts(f, t, srcs, clim if with_clim else None, kidx), srcs)
    table = NB.FractionsTable(NAMES, lat_deg(H), W, n_leads, ev, scales, bands=BANDS,
                              climatology=to_dev(clim) if with_clim else None, **table_kw)
    cnt = FO.counts(f, t, srcs, scales, table.half_x, clim if with_clim else None, kidx)
    kd = None if (kidx is None or not with_clim) else to_dev(np.asarray(kidx, np.int32))
    table.update(lead, (place or to_dev)(f), to_dev(t), kd)
    assert_counts(table, {lead: (cnt, B)})
    return table, cnt


# ================================================================================================ 1. grids
def _grid_cases():
    R = rows(64)
    return [("one row", 1, 8, [0, 1, NY_MAX]), ("a window taller than the grid and exactly as wide", 3, 5, [0, 1, 2]),
            ("5x7", 5, 7, [0, 1, NY_MAX]), ("17x37: the scalar path", 17, 37, [0, 1, NY_MAX]),
            ("headline 32x64", 32, 64, [0, 1, NY_MAX]), ("one workgroup's rows", R, 64, [0, 1, NY_MAX]),
            ("a halo across the workgroup edge", R + 1, 64, [0, 1, NY_MAX]),
            ("the widest row", 40, int(L.paradis_fss_max_w()), [0, 1, NY_MAX])]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", _grid_cases(), ids=lambda c: c[0])
def test_sums_at_grid_edges(case, B):
    """all three source kinds in one launch at every grid edge; ny_max = max_half_y reaches over every workgroup edge"""
    _, H, W, scales = case
    assert rows(64) >= 1 and L.paradis_fss_max_w() >= 1440
    f, t, clim = design(203 + H + W, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    table, cnt = run_design(f, t, clim, None, ev, srcs, scales)
    if (H, W) == (3, 5):
        assert table.half_x[2].tolist() == [2, 2, 2] and (table.window_cells[2] == 15).all()
    assert (cnt["fo"][:, :, -1, 0] > 0).all()


# ================================================================================================ 2. sources, thresholds
SCALES = [0, 2, 5]
SOURCE_CASES = [("plain", ("plain",), None, "ge", SCALES), ("speed", ("speed",), None, "ge", SCALES),
                ("anomaly", ("anomaly",), None, "ge", SCALES), ("T=1", ("plain",), [0.25], "ge", SCALES),
                ("T=3", ("plain", "anomaly"), [0.25, -0.5, 1.25], "ge", SCALES),
                ("T=8 unsorted", ("plain", "anomaly"), THR8, "ge", SCALES),
                ("le", ("plain", "speed", "anomaly"), None, "le", SCALES), ("K=1", ("plain", "speed"), None, "ge", [3]),
                ("K=max", ("plain", "anomaly"), THR8, "ge", [0, 1, 2, 3, 4, 6, 9, NY_MAX][:K_MAX]),
                # (test_hip_events.py's "T=3" and "T=5": threshold counts that events.hip rounds up to a compiled variant)
                ("T=3 speed", ("plain", "speed"), [0.25, -0.5, 1.0], "ge", SCALES),
                ("T=5", ("plain", "anomaly"), THR8[:5], "le", SCALES)]


@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
@pytest.mark.parametrize("case", SOURCE_CASES, ids=lambda c: c[0])
def test_sources_thresholds_and_scales(case, H, W):
    _, kinds, thr, direction, scales = case
    f, t, clim = design(7, 2, H, W, K=2)
    ev, srcs = make_sources(kinds, thr, direction)
    table, _ = run_design(f, t, clim, np.array([1, 0]), ev, srcs, scales)
    assert table.T == max(len(s["thresholds"]) for s in srcs) and len(table.scales) == len(scales)


@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
def test_mixed_and_out_of_range_climatology_slots(H, W):
    """K = 2 with mixed clim_index and one slot out of range: that sample has no event for the anomaly source"""
    f, t, clim = design(11, 3, H, W, K=2)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    table, cnt = run_design(f, t, clim, np.array([1, 2, 0]), ev, srcs, SCALES)
    assert (cnt["valid"][2] == 2 * W).all() and (cnt["valid"][0] == 3 * W).all()
    inside = FO.counts(f[[0, 2]], t[[0, 2]], srcs, SCALES, table.half_x, clim, np.array([1, 0]))
    for k in FO.KEYS:
        assert np.array_equal(cnt[k][2], inside[k][2]), k
    below = NB.FractionsTable(NAMES, lat_deg(H), W, 2, ev, SCALES, bands=BANDS, climatology=to_dev(clim))
    below.update(0, to_dev(f), to_dev(t), torch.tensor([1, -1, 0], dtype=torch.int32).cuda())
    assert torch.equal(below.acc, table.acc)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_cells_are_non_events(bad):
    """NaN / +-Inf at a row end, in a halo row of the next workgroup and at columns 0 / W - 1: the cell leaves nV and
    every window that held it counts one event less"""
    R = rows(64, 3)
    H, W, B = R + 4, 64, 2
    scales = [0, 1, 3]
    f, t, clim = design(31, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    base = FO.counts(f, t, srcs, scales, NB.half_x_table(scales, lat_deg(H), W), clim, None)
    f[0, 0, 2, W - 1] = bad           # plain: forecast, the end of a row (a planted truth-side event cell)
    t[1, 0, R - 1, 0] = bad           # plain: truth, column 0 of the last row of workgroup 0 - a halo row of workgroup 1
    f[1, 2, R, 5] = bad               # speed: second component, the first row of workgroup 1 - a halo row of workgroup 0
    t[0, 1, H - 1, W - 1] = bad       # speed: first component, the last cell of the grid
    f[0, 3, 0, 0] = bad               # anomaly: forecast, the first cell of the grid
    clim[0, 3, R + 1, W - 1] = bad    # anomaly: climatology (both samples read slot 0)
    _, cnt = run_design(f, t, clim, None, ev, srcs, scales, judge=False)
    gone = base["valid"] - cnt["valid"]
    want = np.zeros_like(gone)
    want[0, 2] = want[0, R - 1] = want[1, R] = want[1, H - 1] = want[2, 0] = 1
    want[2, R + 1] = 2
    assert np.array_equal(gone, want)
    # the planted cell (2, W - 1) was a truth event of every plain threshold: 3 x 3 windows in rows 1 .. 3 lose it
    lost = base["oo"][0, :, 1, 0] - cnt["oo"][0, :, 1, 0]
    assert (lost[1:4] > 0).all() and lost[0] == 0 and (lost[4:R - 2] == 0).all()
    assert np.array_equal(base["ff"][0, :R - 2, 1, 0], cnt["ff"][0, :R - 2, 1, 0])     # (it was no forecast event)


# ================================================================================================ 3. against events.hip
@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440), (17, 37)])
def test_scale_zero_equals_the_event_table_on_the_device(H, W):
    """the shared source evaluation (event_source.h) gives the same bits in both kernels: nV, nF, nO are EventTable's, and at ny = nx = 0
    FF == nF, OO == nO, FO == nFO"""
    f, t, clim = design(41, 3, H, W, K=2)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    fd, td, cd = to_dev(f), to_dev(t), to_dev(clim)
    kd = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    events = EV.EventTable(NAMES, lat_deg(H), 1, ev, climatology=cd)
    events.update(0, fd, td, kd)
    fr = NB.FractionsTable(NAMES, lat_deg(H), W, 1, ev, [0, 2], climatology=cd)
    fr.update(0, fd, td, kd)
    a, b = events.counts(), fr.counts()
    assert np.array_equal(a["valid"], b["valid"]) and a["valid"].sum() > 0
    assert np.array_equal(a["forecast_yes"], b["forecast_yes"]) and np.array_equal(a["observed_yes"], b["observed_yes"])
    assert np.array_equal(a["forecast_yes"], b["ff"][:, :, :, 0]) and np.array_equal(a["observed_yes"], b["oo"][:, :, :, 0])
    assert np.array_equal(a["both"], b["fo"][:, :, :, 0]) and a["both"].max() > 0


# ================================================================================================ 4. windows
def test_metric_scaling_with_poles_and_an_explicit_table():
    H, W, B = 33, 64, 2
    lat = np.linspace(-90.0, 90.0, H)
    f, t, clim = design(43, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    cd, fd, td = to_dev(clim), to_dev(f), to_dev(t)
    scales = [0, 1, 4]
    metric = NB.FractionsTable(NAMES, lat, W, 1, ev, scales, lon_scaling="metric", climatology=cd)
    assert metric.half_x[2, 0] == metric.half_x[2, -1] == 31 and metric.half_x[2, 16] == 4
    metric.update(0, fd, td)
    assert_counts(metric, {0: (FO.counts(f, t, srcs, scales, metric.half_x, clim, None), B)})
    hx = np.random.default_rng(5).integers(0, 32, (3, H))
    hx[:, ::3] = 0                                         # the cell's own column on some rows
    hx[1, 1], hx[2, 2] = 31, 31                            # 2 nx + 1 == W - 1
    explicit = NB.FractionsTable(NAMES, lat, W, 1, ev, scales, half_x=hx, climatology=cd)
    explicit.update(0, fd, td)
    assert_counts(explicit, {0: (FO.counts(f, t, srcs, scales, hx, clim, None), B)})


def test_the_kernel_clamps_half_widths_it_cannot_check():
    """half_x lives on the device: an entry outside [0, min(max_half_x, (W - 1) / 2)] is clamped by the kernel (the
    Python side never makes one; here the table is spoilt behind its back before the first upload)"""
    H, W, B = 9, 20, 1
    f, t, clim = design(47, B, H, W)
    ev, srcs = make_sources(("plain",))
    table = NB.FractionsTable(NAMES, lat_deg(H), W, 1, ev, [1, 2])
    table.half_x[0, :] = [-3, 0, 9, 10, 1000, 2 ** 31 - 1, -2 ** 31, 5, 64]
    table.half_x[1, :] = 65
    clamped = np.clip(table.half_x, 0, 9)
    table.update(0, to_dev(f), to_dev(t))
    assert_counts(table, {0: (FO.counts(f, t, srcs, [1, 2], clamped), B)})


def test_forecast_equal_to_truth_is_perfect():
    H, W, B = 17, 37, 2
    _, t, clim = design(53, B, H, W)
    ev, _ = make_sources(("plain", "speed", "anomaly"))
    table = NB.FractionsTable(NAMES, lat_deg(H), W, 1, ev, [0, 1, 4], bands=BANDS, climatology=to_dev(clim))
    table.update(0, to_dev(t), to_dev(t))
    c = table.counts()
    assert np.array_equal(c["ff"], c["oo"]) and np.array_equal(c["ff"], c["fo"]) and c["ff"].max() > 0
    res = table.result()
    live = ~np.isnan(res["fss"])
    assert live.any() and (res["fss"][live] == 1.0).all() and (res["fbs"][live] == 0.0).all()
    assert (table.skilful_scale(res)[~np.isnan(res["fss_uniform"])] == 0).all()


@pytest.mark.parametrize("wf,wo", [(4, 7), (62, 1)], ids=["interior", "across the date line"])
def test_displaced_cell_known_answer_on_the_device(wf, wo):
    """one forecast event cell 3 columns from the one truth cell: fss = max(0, 1 - 3 / (2n + 1))"""
    H, W, scales = 40, 64, [0, 1, 2, 3, 4]
    f, t = np.zeros((1, 4, H, W), np.float32), np.zeros((1, 4, H, W), np.float32)
    f[0, 0, 20, wf] = t[0, 0, 20, wo] = 1.0
    ev = {"rain": {"source": "tp", "thresholds": [0.5]}}
    table = NB.FractionsTable(NAMES, lat_deg(H), W, 1, ev, scales, weights=np.ones(H))
    table.update(0, to_dev(f), to_dev(t))
    res = table.result()
    np.testing.assert_allclose(res["fss"][0, 0, 0, :, 0], [0.0, 0.0, 0.4, 4.0 / 7.0, 2.0 / 3.0], rtol=1e-12, atol=0)
    c = table.counts()
    for k, n in enumerate(scales):
        assert c["ff"][0, 0, :, k, 0].sum() == c["oo"][0, 0, :, k, 0].sum() == (2 * n + 1) ** 2
        assert c["fo"][0, 0, :, k, 0].sum() == (2 * n + 1) * max(0, 2 * n + 1 - 3)
    assert table.skilful_scale(res)[0, 0, 0, 0] == 3        # 4 / 7 >= 0.5 + (1 / 2560) / 2


# ================================================================================================ 5. layouts
@pytest.mark.parametrize("H,W", [(32, 64), (6, 1440)])
def test_offset_and_strided_views_equal_dense(H, W):
    B = 2
    f, t, clim = design(17, B, H, W)
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    dense, _ = run_design(f, t, clim, None, ev, srcs, SCALES)

    def offset(x):
        buf = torch.zeros(x.size + 1, device="cuda")
        view = buf[1:].view(*x.shape)
        view.copy_(torch.from_numpy(x))
        assert view.data_ptr() % 16 == 4
        return view

    shifted, _ = run_design(f, t, clim, None, ev, srcs, SCALES, place=offset, judge=False)
    assert torch.equal(shifted.acc, dense.acc) and torch.equal(shifted.n_samples, dense.n_samples)
    chunk = torch.full((B, 3, 4, H, W), float("nan"), device="cuda")
    true = torch.full((B, 3, 4, H, W), float("nan"), device="cuda")
    chunk[:, 1], true[:, 1] = to_dev(f), to_dev(t)
    table = NB.FractionsTable(NAMES, lat_deg(H), W, 2, ev, SCALES, bands=BANDS, climatology=to_dev(clim))
    table.update(0, chunk[:, 1], true[:, 1])
    assert torch.equal(table.acc, dense.acc)
    odd = torch.zeros(B, 4 * H * W + 1, device="cuda")[:, :4 * H * W].view(B, 4, H, W)     # a batch stride of 4 k + 1
    odd.copy_(to_dev(f))
    table.reset()
    table.update(0, odd, true[:, 1])
    assert torch.equal(table.acc, dense.acc)


# ================================================================================================ 6. accumulation
def test_accumulation_leads_and_repeats():
    H, W = 6, 1440
    f, t, clim = design(23, 5, H, W, K=2)
    kidx = np.array([0, 1, 1, 0, 1])
    ev, srcs = make_sources(("plain", "speed", "anomaly"))
    fd, td, kd, cd = to_dev(f), to_dev(t), to_dev(kidx.astype(np.int32)), to_dev(clim)

    def fresh():
        return NB.FractionsTable(NAMES, lat_deg(H), W, 3, ev, SCALES, bands=BANDS, climatology=cd)

    a, b, c = fresh(), fresh(), fresh()
    cnt = FO.counts(f, t, srcs, SCALES, a.half_x, clim, kidx)
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
    b.update(1, fd, td, kd)
    assert torch.equal(b.acc, 2 * a.acc) and b.n_samples.tolist() == [0, 10, 0]  # two updates double the sums
    b.update(2, fd, td, kd)
    assert torch.equal(b.acc[2], a.acc[1]) and torch.equal(b.acc[1], 2 * a.acc[1]) and b.n_samples.tolist() == [0, 10, 5]
    d = fresh()
    d.acc[1].fill_(2 ** 32 - 1)
    d.update(1, fd, td, kd)
    assert torch.equal(d.acc[1] - (2 ** 32 - 1), a.acc[1]) and int(d.acc[1].max()) > 2 ** 32     # the carry into the upper word
    a.reset()
    assert int(a.acc.abs().sum()) == 0 and int(a.n_samples.sum()) == 0


def test_update_refusals_on_the_device():
    H, W = 4, 8
    ev, _ = make_sources(("plain",))
    table = NB.FractionsTable(NAMES, lat_deg(H), W, 1, ev, [0, 1])
    x = torch.zeros(2, 4, H, W, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        table.update(0, x.cpu(), x)
    with pytest.raises(ValueError, match="dense"):
        table.update(0, torch.zeros(2, 4, H, 2 * W, device="cuda")[..., ::2], x)
    cpu_table = NB.FractionsTable(NAMES, lat_deg(H), W, 1, ev, [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu_table.update(0, x, x)
    # what only the entry point refuses (rc 1, before any HIP call) comes back as a ValueError
    wide = int(L.paradis_fss_max_w()) + 4
    too_wide = NB.FractionsTable(NAMES, lat_deg(2), wide, 1, ev, [0, 1])
    y = torch.zeros(1, 4, 2, wide, device="cuda")
    with pytest.raises(ValueError, match="longitudes"):
        too_wide.update(0, y, y)
    table._half_y = np.array([0, NY_MAX + 1], np.int32)
    with pytest.raises(ValueError, match="half_y"):
        table.update(0, x, x)
    assert int(table.acc.abs().sum()) == 0 and int(too_wide.acc.abs().sum()) == 0 and int(table.n_samples.sum()) == 0


# ================================================================================================ 7. integration
def test_update_is_graph_capturable():
    """an update captured in a HIP graph and replayed twice equals two eager updates"""
    from paradis_model_amd.harness import capture_forward
    B, H, W = 2, 32, 64
    f, t, clim = design(29, B, H, W, K=2)
    ev, _ = make_sources(("plain", "speed", "anomaly"))
    fd, td, cd = to_dev(f), to_dev(t), to_dev(clim)
    kd = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    eager = NB.FractionsTable(NAMES, lat_deg(H), W, 2, ev, SCALES, climatology=cd)
    eager.update(1, fd, td, kd)
    eager.update(1, fd, td, kd)
    graphed = NB.FractionsTable(NAMES, lat_deg(H), W, 2, ev, SCALES, climatology=cd)
    graph, _ = capture_forward(lambda: graphed.update(1, fd, td, kd), warmup=1)
    torch.cuda.synchronize()
    graphed.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.acc, eager.acc) and graphed.n_samples.tolist() == [0, 2 * B]
    assert int(eager.acc[1].abs().sum()) > 0


@pytest.mark.parametrize("truth_normalized,graph,with_card", [(False, False, False), (True, True, True)])
def test_forecaster_hook(truth_normalized, graph, with_card):
    """run(fractions=..., truth=...) updates with the chunks it hands to on_chunk: bit for bit the accumulators of a table
    updated by hand with those chunks; the chunks are those of a run without a table; beside a scorecard both get the
    same states and the same clim_index column"""
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.verify import Scorecard
    from tests import forecast_oracle as FCO
    from tests.test_hip_verify import _Collect, _rollout_setup, lat_weights
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    C = spec.num_channels
    norm = FCO.normalised_state(31, spec.names, B, S, C, H, W).cuda()
    phys = torch.empty(B, S, C, H, W, device="cuda")
    clim = torch.empty(1, 2, C, H, W, device="cuda")
    cnorm = FCO.normalised_state(32, spec.names, 1, 2, C, H, W).cuda()
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

    def fresh(n_leads=S):
        return NB.FractionsTable(spec.names, lat, W, n_leads, ev, [0, 1, 3], lon_scaling="metric",
                                 bands={"sh": (-90.0, 0.0), "nh": (0.0, 90.0)}, climatology=clim)

    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=graph)
    plain = _Collect()
    fc.run(*inputs, plain)
    table = fresh()
    card = Scorecard(spec.names, lat_weights(H), S, climatology=clim) if with_card else None
    scored = _Collect()
    fc.run(*inputs, scored, fractions=table, scorecard=card, truth=norm if truth_normalized else phys,
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
    assert (cnt["valid"] == B * W).all() and (cnt["oo"][:, 0, :, :, 0].sum(axis=(0, 1)) > 0).all()
    if with_card:
        alone = Scorecard(spec.names, lat_weights(H), S, climatology=clim)
        fc.run(*inputs, None, scorecard=alone, truth=norm if truth_normalized else phys,
               truth_normalized=truth_normalized, clim_index=kidx)
        assert torch.equal(card.acc, alone.acc)
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, fractions=table, truth=phys[:, :2])           # a wrong n_stored: before the rollout
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, fractions=table)
    with pytest.raises(ValueError, match="leads"):
        fc.run(*inputs, None, fractions=fresh(S - 1), truth=phys)
    assert torch.equal(table.acc, by_hand.acc)
