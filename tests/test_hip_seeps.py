"""GPU: the SEEPS update (paradis_model_amd/seeps.py ``SeepsTable``, csrc/seeps.hip ``paradis_seeps_update``) against the
numpy restatement of tests/seeps_oracle.py, on the designs of tests/seeps_cases.py.

Shapes come from ``paradis_seeps_rows(W)`` (tests/test_seeps_cpu.py asserts what each reaches): (B=3, H=5, W=10) scalar
path, a partial walk, K = 3 slots, Cs = 2 channels; (B=2, H=33, W=260) vector path, two walks per row, row groups of
31 + 2; (B=2, H=6, W=7) odd width; (B=1, H=2, W=512) two full walks.

Bounds.  The counters equal the oracle's exactly.  A row's double sums are sums of the same non-negative terms in
another order (lanes, then the xor tree, then samples), so |device - oracle| <= n_row * 2^-52 * sum with n_row the row's
valid cells: derived, not measured.  A row with exactly ONE valid cell shows that cell's ``s`` itself - the divisions
included -, and there device and oracle agree bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import seeps_cases as SC
from tests import seeps_oracle as SO

pytestmark = pytest.mark.gpu

DESIGNS = list(SC.UPDATE_SHAPES)


def _lat(H):
    return np.linspace(-80.0, 80.0, H)


def _names(C):
    return [f"x{c}" for c in range(C)]


def _table(name, data, n_leads=1, **kw):
    """a table over the design's state layout with ``data`` [2, K, Cs, H, W] (numpy) as its climatology"""
    from paradis_model_amd.climatology import SeepsClimatology
    from paradis_model_amd.seeps import SeepsTable
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    names = _names(Cs + 1)
    chan = [Cs - cs for cs in range(Cs)]
    clim = SeepsClimatology(_dev(data), None, [names[c] for c in chan], SC.DRY)
    return SeepsTable(names, _lat(H), n_leads, clim, p1_bounds=(SC.P_LO, SC.P_HI), **kw)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # (a copy: the cases are read-only)


@functools.lru_cache(maxsize=None)
def _want(name, want=0):
    fc, tr, data, idx, chan, C = SC.update_case(name, want)
    real, ints, cells = SO.rows(fc, tr, data, idx, chan, SC.DRY, SC.P_LO, SC.P_HI)
    real.setflags(write=False)
    ints.setflags(write=False)
    return real, ints, cells


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_rows(cnt, real, ints, what, lead=0):
    """the integers exactly; every double row sum within n_row 2^-52 of the oracle's"""
    got_i = np.concatenate([cnt["table"][lead].reshape(ints.shape[:-1] + (9,)), cnt["masked"][lead][..., None]], axis=-1)
    assert np.array_equal(got_i, ints), what
    n_row = ints[..., :9].sum(axis=-1).astype(np.float64)[..., None]
    err = np.abs(cnt["sums"][lead] - real)
    bound = n_row * 2.0 ** -52 * real
    print(f"SEEPS {what} | worst row-sum error / bound {float((err / np.where(bound > 0, bound, 1.0)).max()):.3g}")
    assert bool((err <= bound).all()), f"{what}: {float((err - bound).max())}"


@pytest.mark.parametrize("name", DESIGNS)
def test_counts_sums_and_single_cells_against_the_oracle(name):
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    h = SC.EXACT_ROW[name]
    seen = set()
    for want in range(3):
        fc, tr, data, idx, chan, C = SC.update_case(name, want)
        table = _table(name, data)
        assert table.index == chan
        table.update(0, _dev(fc), _dev(tr), _dev(idx))
        cnt = table.counts()
        real, ints, cells = _want(name, want)
        _assert_rows(cnt, real, ints, f"{name} truth category {want}")
        assert int(cnt["n_samples"][0]) == B
        for cs in range(Cs):                          # the row of one valid cell: its s, divisions included, bit for bit
            (b, w, cf, co, s), = cells[(cs, h)]
            assert (b, co, cf) == (0, want, (want + 1) % 3) and s > 0.0
            expect = np.zeros(3)
            expect[co] = s
            assert np.array_equal(_bits64(cnt["sums"][0, cs, h]), _bits64(expect)), (name, want, cs)
            assert int(cnt["table"][0, cs, h].sum()) == 1 and int(cnt["table"][0, cs, h, cf, co]) == 1
            seen.add(co)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("name", DESIGNS)
def test_views_equal_the_dense_run_bit_for_bit(name):
    """an offset of one element (unaligned: scalar loads whatever W is) and a batch-strided view of a [B, C + 1, H, W]
    buffer give the dense run's integers and doubles"""
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, idx, chan, C = SC.update_case(name)
    dense = _table(name, data)
    dense.update(0, _dev(fc), _dev(tr), _dev(idx))
    n = B * C * H * W
    off_f, off_t = torch.zeros(n + 1, device="cuda"), torch.zeros(n + 1, device="cuda")
    off_f[1:] = _dev(fc).reshape(-1)
    off_t[1:] = _dev(tr).reshape(-1)
    shifted = _table(name, data)
    shifted.update(0, off_f[1:].view(B, C, H, W), off_t[1:].view(B, C, H, W), _dev(idx))
    wide_f, wide_t = torch.full((B, C + 1, H, W), 7.0, device="cuda"), torch.full((B, C + 1, H, W), 7.0, device="cuda")
    wide_f[:, 1:] = _dev(fc)
    wide_t[:, :C] = _dev(tr)
    strided = _table(name, data)
    strided.update(0, wide_f[:, 1:], wide_t[:, :C], _dev(idx))
    assert wide_f[:, 1:].stride(0) == (C + 1) * H * W and off_f[1:].data_ptr() % 16 == 4
    for other in (shifted, strided):
        assert torch.equal(other.acc_int, dense.acc_int) and torch.equal(other.n_samples, dense.n_samples)
        assert torch.equal(other.acc_real.view(torch.int64), dense.acc_real.view(torch.int64))
    assert int(dense.acc_int.sum()) > 0


def test_mixed_and_out_of_range_slots_and_two_channels():
    name = "small"
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, idx, chan, C = SC.update_case(name)
    assert K == 3 and Cs == 2 and len(set(idx.tolist())) == 3
    for bad in (K, -1, 2 ** 30):
        idx2 = idx.copy()
        idx2[1] = bad
        table = _table(name, data)
        table.update(0, _dev(fc), _dev(tr), _dev(idx2))
        real, ints, _ = SO.rows(fc, tr, data, idx2, chan, SC.DRY, SC.P_LO, SC.P_HI)
        cnt = table.counts()
        _assert_rows(cnt, real, ints, f"slot {bad}")
        # the sample adds nothing anywhere: the table of the other two samples alone
        keep = [0, 2]
        alone = _table(name, data)
        alone.update(0, _dev(fc[keep]), _dev(tr[keep]), _dev(idx[keep]))
        assert torch.equal(alone.acc_int, table.acc_int)
        assert torch.equal(alone.acc_real.view(torch.int64), table.acc_real.view(torch.int64))
        assert int(cnt["n_samples"][0]) == B and int(alone.n_samples[0]) == 2
    both = _want(name)[1]
    assert bool((both[0].sum(axis=0) != both[1].sum(axis=0)).any())              # the two channels differ


def test_ties_and_non_finite_inputs():
    """f == thr is heavy, o == dry is not dry; a NaN or an Inf in any of the four inputs takes the cell out of every
    class"""
    name = "small"
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, idx, chan, C = SC.update_case(name)
    real, ints, cells = _want(name)
    k0, c0 = int(idx[0]), chan[0]
    tie_f = [(b, w) for (b, w, cf, co, s) in cells[(0, 0)] if b == 0 and fc[0, c0, 0, w] == data[1, k0, 0, 0, w]]
    tie_o = [(w, co) for (b, w, cf, co, s) in cells[(0, 0)] if b == 0 and tr[0, c0, 0, w] == np.float32(SC.DRY)]
    assert len(tie_f) == 1 and len(tie_o) == 1 and tie_o[0][1] >= 1
    assert [cf for (b, w, cf, co, s) in cells[(0, 0)] if (b, w) == tie_f[0]] == [2]
    base = _table(name, data)
    base.update(0, _dev(fc), _dev(tr), _dev(idx))
    base_total = int(base.acc_int.sum())
    inside = SO.classes(data, SC.P_LO, SC.P_HI)["inside"]
    h = 2
    w = int(np.flatnonzero(inside[k0, 0, h] & np.isfinite(fc[0, c0, h]) & np.isfinite(tr[0, c0, h]))[0])
    for which in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            f2, t2, d2 = fc.copy(), tr.copy(), data.copy()
            (f2[0, c0, h], t2[0, c0, h], d2[0, k0, 0, h], d2[1, k0, 0, h])[which][w] = bad
            table = _table(name, d2)
            table.update(0, _dev(f2), _dev(t2), _dev(idx))
            r2, i2, _ = SO.rows(f2, t2, d2, idx, chan, SC.DRY, SC.P_LO, SC.P_HI)
            _assert_rows(table.counts(), r2, i2, f"input {which} {bad}")
            assert int(table.acc_int.sum()) == base_total - 1


def test_bit_level_promises():
    """two updates equal one update of the concatenated batch; a rerun equals itself; reset() clears"""
    name = "groups"
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, idx, chan, C = SC.update_case(name)
    f, t, i = _dev(fc), _dev(tr), _dev(idx)
    whole = _table(name, data, n_leads=2)
    whole.update(1, f, t, i)
    parts = _table(name, data, n_leads=2)
    parts.update(1, f[:1], t[:1], i[:1])
    parts.update(1, f[1:], t[1:], i[1:])
    again = _table(name, data, n_leads=2)
    again.update(1, f, t, i)
    for other in (parts, again):
        assert torch.equal(other.acc_int, whole.acc_int) and torch.equal(other.n_samples, whole.n_samples)
        assert torch.equal(other.acc_real.view(torch.int64), whole.acc_real.view(torch.int64))
    assert whole.n_samples.tolist() == [0, B] and int(whole.acc_int[0].sum()) == 0 and float(whole.acc_real[0].sum()) == 0.0
    whole.update(1, f, t, i)                                        # accumulates
    assert torch.equal(whole.acc_int[1], 2 * again.acc_int[1]) and whole.n_samples.tolist() == [0, 2 * B]
    whole.reset()
    assert int(whole.acc_int.sum()) == 0 and float(whole.acc_real.abs().sum()) == 0.0 and whole.n_samples.tolist() == [0, 0]
    whole.update(1, f, t, i)
    assert torch.equal(whole.acc_real.view(torch.int64), again.acc_real.view(torch.int64))


def test_result_against_the_oracles_report():
    name = "small"
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, idx, chan, C = SC.update_case(name)
    bands = {"global": (-90.0, 90.0), "north": (0.0, 90.0)}
    table = _table(name, data, n_leads=2, bands=bands)
    table.update(1, _dev(fc), _dev(tr), _dev(idx))
    res = table.result()
    real, ints, _ = _want(name)
    zero_r, zero_i = np.zeros_like(real), np.zeros_like(ints)
    want = SO.report(np.stack([zero_r, real]), np.stack([zero_i, ints]), np.array([0, B]), table.band_w)
    for k, v in want.items():
        assert res[k].shape == v.shape and np.array_equal(np.isnan(res[k]), np.isnan(v)), k
        assert np.allclose(res[k], v, rtol=1e-12, atol=0.0, equal_nan=True), k
    assert bool(np.isnan(res["seeps"][0]).all()) and bool(np.isfinite(res["seeps"][1]).all())
    assert bool((res["seeps"][1] > 0).all()) and bool((res["coverage"][1] < 1).all()) and res["count"].tolist() == [0, B]
    assert res["names"] == table.names and res["bands"] == ["global", "north"]
    assert "north" in table.table(res, table.names[1], "north")


def test_update_refusals_on_the_device():
    name = "odd"
    B, H, W, K, Cs = SC.UPDATE_SHAPES[name]
    fc, tr, data, idx, chan, C = SC.update_case(name)
    table = _table(name, data)
    f, t = _dev(fc), _dev(tr)
    table.update(0, f, t)                                           # one slot: clim_index is optional
    with_index = _table(name, data)
    with_index.update(0, f, t, _dev(idx))
    assert torch.equal(table.acc_int, with_index.acc_int)
    with pytest.raises(ValueError, match="live on the device"):
        table.update(0, f, t, torch.from_numpy(idx.copy()))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        table.update(0, f.cpu(), t)
    before = table.acc_int.clone()
    table.update(0, f[:0], t[:0], _dev(idx)[:0])                    # an empty batch does nothing
    assert torch.equal(table.acc_int, before)


# ---------------------------------------------------------------------------------- end to end
def test_build_seeps_into_the_table_with_the_stores_own_rows_as_truth():
    """the climatology of a (6, 10) store, truth rows taken from the store: a perfect forecast scores exactly 0; the
    constant forecasts "always dry" and "always heavy" score what the oracle gives for the same cells"""
    from paradis_model_amd import climatology
    from paradis_model_amd.seeps import SeepsTable
    from tests.test_hip_seeps_clim import PLANS, _decoded, _store
    grid = SC.CLIM_GRIDS[0]
    H, W = grid
    store = _store(grid, None)
    plan = climatology.ClimPlan(store.times_us, **PLANS["w61"])
    names = ["total_precipitation_6hr"]
    sc = climatology.build_seeps(store, plan, names, SC.DRY)
    rows = [62, 181, 460, 1]                   # 1 Jan 00 h, 29 Feb 12 h (day 60), 18 Jul 00 h (day 200); and a day not built
    times = store.times_us.numpy()[rows[:3]]
    idx = torch.cat([sc.index(times), torch.tensor([plan.n_slots], dtype=torch.int32, device="cuda")])
    assert sorted(set(idx.tolist())) == sorted(idx.tolist()) and len(rows) == 4
    x = _decoded(grid, None)
    state = ["temperature_h850"] + names                            # the state's channels; the second one is scored
    truth = np.ascontiguousarray(x[rows][:, [SC.FEATURES.index(n) for n in state]])  # [4, 2, H, W]
    data = sc.data.cpu().numpy()
    lat = np.linspace(-75.0, 75.0, H)
    heavy = truth.copy()                                            # f = thr: heavy
    heavy[:, 1] = np.where(np.isfinite(data[1]), data[1], 1.0)[idx.cpu().numpy().clip(0, plan.n_slots - 1), 0]
    forecasts = {"perfect": truth, "dry": np.zeros_like(truth), "heavy": heavy}
    for kind, fc in forecasts.items():
        table = SeepsTable(state, lat, 1, sc)
        table.update(0, _dev(fc), _dev(truth), idx)
        cnt, res = table.counts(), table.result()
        real, ints, _ = SO.rows(fc, truth, data, idx.cpu().numpy(), [1], SC.DRY)
        _assert_rows(cnt, real, ints, kind)
        want = SO.report(real[None], ints[None], np.array([4]), table.band_w)
        assert np.allclose(res["seeps"], want["seeps"], rtol=1e-12, atol=0.0) and int(ints[..., :9].sum()) > 50
        pairs = ints[..., :9].sum(axis=(0, 1)).reshape(3, 3)
        if kind == "perfect":
            assert float(np.abs(cnt["sums"]).max()) == 0.0 and float(res["seeps"][0, 0, 0]) == 0.0
            assert float(res["seeps_skill"][0, 0, 0]) == 1.0 and int(pairs.sum()) == int(np.trace(pairs))
            assert bool((np.diag(pairs) > 0).all())
        else:
            row = 0 if kind == "dry" else 2
            assert int(pairs.sum()) == int(pairs[row].sum()) and bool((pairs[row] > 0).all())
            assert 0.0 < float(res["seeps"][0, 0, 0]) and np.isclose(res["forecast_freq"][0, 0, 0, row], 1.0, rtol=1e-14)
        assert 0.0 < float(res["coverage"][0, 0, 0]) < 1.0


def test_forecaster_hook():
    """run(seeps=..., truth=...) scores the chunks it hands to on_chunk: bit for bit the accumulators of a table updated
    by hand with those chunks, beside an event table that gets the same clim_index column"""
    from paradis_model_amd.climatology import SeepsClimatology
    from paradis_model_amd.events import EventTable
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.seeps import SeepsTable
    from tests import forecast_oracle as FO
    from tests.test_hip_verify import _Collect, _rollout_setup
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    C = spec.num_channels
    norm = FO.normalised_state(31, spec.names, B, S, C, H, W).cuda()
    phys = torch.empty(B, S, C, H, W, device="cuda")
    for s in range(S):
        postprocess(norm[:, s], spec, lat, lon, phys, s)
    chans = [spec.names[-1], spec.names[0]]
    g = torch.Generator().manual_seed(5)
    data = torch.empty(2, 2, 2, H, W)
    data[0] = 0.02 + 0.96 * torch.rand(2, 2, H, W, generator=g)             # p1 on both sides of the bounds
    for j, n in enumerate(chans):
        col = phys[:, :, spec.names.index(n)].cpu()
        data[1, :, j] = float(col.median()) + 0.5 * float(col.std()) * torch.rand(2, H, W, generator=g)
    dry = float(np.float32(phys[:, :, spec.names.index(chans[0])].median().item() - 1.0))
    clim = SeepsClimatology(data.cuda(), None, chans, dry)
    kidx = torch.tensor([[0, 1, 1], [1, 0, 1]], dtype=torch.int32, device="cuda")

    def fresh():
        return SeepsTable(spec.names, lat, S, clim, bands={"sh": (-90.0, 0.0), "nh": (0.0, 90.0)})

    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=True)
    plain = _Collect()
    fc.run(*inputs, plain)
    table = fresh()
    events = EventTable(spec.names, lat, S, {"a": {"source": ("anomaly", chans[0]), "thresholds": [0.0]}},
                        climatology=phys[0, :2].contiguous())
    scored = _Collect()
    fc.run(*inputs, scored, seeps=table, events=events, truth=phys, clim_index=kidx)
    assert [c[0] for c in scored.chunks] == [0, 2] and [c[1].shape[1] for c in scored.chunks] == [2, 1]
    for (s0, x), (s1, y) in zip(plain.chunks, scored.chunks):
        assert s0 == s1 and torch.equal(x, y)                               # the chunk contents are unchanged
    states = torch.cat([c[1] for c in scored.chunks], dim=1)
    by_hand = fresh()
    for s in range(S):
        by_hand.update(s, states[:, s].cuda(), phys[:, s], kidx[:, s].contiguous())
    assert torch.equal(table.acc_int, by_hand.acc_int) and torch.equal(table.n_samples, by_hand.n_samples)
    assert torch.equal(table.acc_real.view(torch.int64), by_hand.acc_real.view(torch.int64))
    assert table.n_samples.tolist() == [B] * S and events.n_samples.tolist() == [B] * S
    cnt = table.counts()
    assert int(cnt["table"].sum()) > 0 and int(cnt["masked"].sum()) > 0
    assert bool((cnt["table"].sum(axis=(3, 4)) + cnt["masked"] == B * W).all())
    with pytest.raises(ValueError, match="a SEEPS table needs truth"):
        fc.run(*inputs, None, seeps=table)
    with pytest.raises(ValueError, match="the SEEPS table has"):
        fc.run(*inputs, None, seeps=SeepsTable(spec.names, lat, S - 1, clim), truth=phys)
    assert torch.equal(table.acc_int, by_hand.acc_int)
