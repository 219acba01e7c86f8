"""GPU: the SEEPS climatology (paradis_model_amd/climatology.py ``clim_seeps`` / ``build_seeps``, csrc/quantile.hip
``paradis_clim_seeps`` / ``paradis_clim_seeps_packed``) against the numpy restatement of tests/seeps_oracle.py.

Stores (tests/seeps_cases.py): three features over the 857 times of ``clim_oracle.case_times``, float32 and
``packing="u16"``, the oracle fed ``store.rows(0, T).cpu()``; the precipitation ramps from always wet in the first
column(s) to always dry in the last; pixel (0, 1) NaN in every third row, pixel (H - 1, W - 2) NaN in every row, pixel
(1, 0) +Inf in every fifth row; one cell whose values all equal the dry threshold (strict comparison: all wet) and one
with exactly one wet value in every hand-made list.

Grids as tests/test_hip_quantile.py: (6, 10) vector path, one partial tile; (5, 7) odd, scalar path; (7, 20) two tiles
and a tail.  Hand-made unsorted lists of 0, 1, 2, 3, 9, 61, 128, 129 and 257 entries - 257 entries take the 128 KiB LDS
tile, which a launch gets only when this instantiation's dynamic shared memory limit was raised -, one launch with
``max_entries=1024`` (32-cell tiles) and one wide-tile launch (``max_entries=16``, 1024 cells) on (33, 64).

Bound: none.  The sort is exact, the rest is IEEE double divide, multiply, subtract, add, floor and one rounding,
uncontracted on both sides: both planes equal the oracle's bit for bit (as uint32), NaN exactly where it has NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import clim_oracle as CO
from tests import forecast_oracle as FO
from tests import seeps_cases as SC
from tests import seeps_oracle as SO

pytestmark = pytest.mark.gpu

GRIDS = SC.CLIM_GRIDS
WIDE_GRID = (33, 64)
WET_LEVELS = [0.0, 2.0 / 3.0, 1.0]
PLANS = {
    "w1": dict(start="2019-12-01", end="2020-12-30", window_days=1),
    "w61": dict(days=[1, 60, 200, 366], window_days=61),
}


def test_shapes_sit_on_the_kernel_edges():
    from paradis_model_amd import _lib
    cells = _lib.lib.paradis_clim_quantile_cells
    assert cells(max(SC.SHORT)) == 64 and max(SC.SHORT) == 257
    assert 64 * 512 * 4 == 128 * 1024 > 64 * 1024                         # the tile of 257 entries: above the default limit
    assert cells(1024) == 32 and cells(16) == 1024
    P = [h * w for h, w in GRIDS]
    assert P[0] < 64 and P[0] % 4 == 0 and P[1] % 4 != 0 and P[2] > 2 * 64 and P[2] % 64 == 12 and P[2] % 4 == 0
    Pw = WIDE_GRID[0] * WIDE_GRID[1]
    assert Pw > 2 * 1024 and Pw % 1024 == 64 and 60 % 32 != 0


@functools.lru_cache(maxsize=None)
def _times():
    t = CO.case_times()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _store(grid, packing):
    from paradis_model_amd.dataset import DeviceStore
    H, W = grid
    lat, lon = FO.grid_deg(H, W, False)
    F = len(SC.FEATURES)
    stats = {k: np.ones(F, np.float32) for k in ("mean", "std", "min", "max")}
    return DeviceStore(SC.store_data(grid, _times().size).copy(), _times(), SC.FEATURES, stats, lat, lon,
                       np.zeros((H, W, 1), np.float32), toa_mean=0.0, toa_std=1.0, device="cuda", packing=packing)


@functools.lru_cache(maxsize=None)
def _decoded(grid, packing):
    """what the store holds, as float32 numpy: the oracle's input, read once and never written"""
    store = _store(grid, packing)
    x = store.rows(0, store.shape[0]).cpu().numpy()
    x.setflags(write=False)
    return x


def _cols(names):
    return [SC.FEATURES.index(n) for n in names]


def _run(store, lists, cols, dry=SC.DRY, rows=None, **kw):
    from paradis_model_amd.climatology import clim_seeps
    dev = store.device
    ptr, r = SO.csr([[(int(e), 1.0) for e in l] for l in lists])[:2]
    rows = np.asarray(r if rows is None else rows, np.int64)
    out, flag = clim_seeps(store, torch.from_numpy(np.asarray(ptr, np.int64)).to(dev), torch.from_numpy(rows).to(dev),
                           torch.tensor(cols, dtype=torch.int32, device=dev), dry, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(flag.item())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    """bit for bit as uint32, NaN exactly where the oracle has NaN"""
    assert got.shape == want.shape and got.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"


@functools.lru_cache(maxsize=None)
def _want_short(grid, packing, wet_level, min_count=1):
    x = _decoded(grid, packing)
    lists = SC.hand_lists(x.shape[0], tuple(SC.SHORT), 31)
    want = SO.slot_climatology(x, lists, _cols(SC.PICK), SC.DRY, wet_level, min_count)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("packing", [None, "u16"])
@pytest.mark.parametrize("grid", GRIDS)
def test_list_lengths_bit_for_bit(grid, packing):
    store = _store(grid, packing)
    H, W = grid
    lists = SC.hand_lists(store.shape[0], tuple(SC.SHORT), 31)
    cols = _cols(SC.PICK)
    for wet_level in WET_LEVELS:
        got, flag = _run(store, lists, cols, wet_level=wet_level, max_entries=max(SC.SHORT))
        assert flag == 0 and got.shape == (2, len(SC.SHORT), len(SC.PICK), H, W)
        _assert_same(got, _want_short(grid, packing, wet_level), f"{grid} {packing} {wet_level}")
    got, _ = _run(store, lists, cols, max_entries=max(SC.SHORT))                    # the default level
    _assert_same(got, _want_short(grid, packing, WET_LEVELS[1]), "default wet_level")
    assert bool(np.isnan(got[:, 0]).all())                                          # the empty list
    assert bool(np.isnan(got[:, :, :, H - 1, W - 2]).all())                         # the all-missing pixel
    assert not bool((_bits(got) == 0x80000000).any())
    t = SC.PICK.index("temperature_h850")                                           # 250 K is never dry
    assert bool((got[0, 1:, t, 2, 2] == 0).all()) and bool((got[1, 1:, t, 2, 2] > 200).all())
    if packing is None:
        # every class of cell is there, and most cells are inside the bounds (tests/test_seeps_cpu.py asserts the same
        # of the oracle's output)
        for n in SC.DESIGN_LISTS:
            cl = SO.classes(got[:, SC.SHORT.index(n), :2], SC.P_LO, SC.P_HI)
            assert all(int(v.sum()) >= 1 for v in cl.values()) and cl["inside"].mean() >= 0.5, n
        k = [i for i, n in enumerate(SC.SHORT) if n]
        h, w = SC.CELL_ALL_AT_DRY                                                   # x == dry is not dry
        assert bool((got[0, k, :2, h, w] == 0).all()) and bool((got[1, k, :2, h, w] == np.float32(SC.DRY)).all())
        h, w = SC.CELL_ONE_WET
        for i in k:
            assert bool((got[0, i, :2, h, w] == np.float32((SC.SHORT[i] - 1) / SC.SHORT[i])).all())
            assert bool((got[1, i, :2, h, w] == np.float32(2e-3)).all())
    # min_count = 3 turns the cells of the 1- and 2-entry lists into NaN, and cells that kept fewer, and nothing else
    got3, flag = _run(store, lists, cols, max_entries=max(SC.SHORT), min_count=3)
    _assert_same(got3, _want_short(grid, packing, WET_LEVELS[1], 3), "min_count=3")
    assert flag == 0 and bool(np.isnan(got3[:, SC.SHORT.index(2)]).all()) and bool(np.isnan(got3[:, SC.SHORT.index(1)]).all())
    assert bool(np.isfinite(got3[0, SC.SHORT.index(3), 0, 2, 2]))
    same = ~np.isnan(got3)
    assert np.array_equal(_bits(got3[same]), _bits(got[same]))
    # two runs: equal bit for bit
    again, _ = _run(store, lists, cols, max_entries=max(SC.SHORT))
    assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("packing", [None, "u16"])
def test_long_lists_under_the_32_cell_tile(packing):
    grid = GRIDS[0]
    store = _store(grid, packing)
    lists = SC.hand_lists(store.shape[0], (600, 5), 32)
    cols = _cols(SC.PICK[:2])
    got, flag = _run(store, lists, cols, max_entries=1024)
    assert flag == 0
    _assert_same(got, SO.slot_climatology(_decoded(grid, packing), lists, cols, SC.DRY), f"{packing}")
    got2, flag = _run(store, lists, cols)                         # the default tile (4096 entries, 8 cells): the same bits
    assert flag == 0 and np.array_equal(_bits(got2), _bits(got))


@pytest.mark.parametrize("packing", [None, "u16"])
def test_short_lists_under_the_wide_tile(packing):
    store = _store(WIDE_GRID, packing)
    lists = SC.hand_lists(store.shape[0], (9, 16, 4), 33)
    cols = _cols(SC.PICK[:1])
    got, flag = _run(store, lists, cols, max_entries=16)
    assert flag == 0
    _assert_same(got, SO.slot_climatology(_decoded(WIDE_GRID, packing), lists, cols, SC.DRY), f"{packing}")


def test_packed_store_equals_the_float32_store_of_its_decoded_rows():
    from paradis_model_amd.dataset import DeviceStore
    grid = GRIDS[1]
    H, W = grid
    packed = _store(grid, "u16")
    lat, lon = FO.grid_deg(H, W, False)
    stats = {k: np.ones(len(SC.FEATURES), np.float32) for k in ("mean", "std", "min", "max")}
    plain = DeviceStore(_decoded(grid, "u16").copy(), _times(), SC.FEATURES, stats, lat, lon,
                        np.zeros((H, W, 1), np.float32), toa_mean=0.0, toa_std=1.0, device="cuda", packing=None)
    lists = SC.hand_lists(packed.shape[0], tuple(SC.SHORT), 31)
    a, _ = _run(packed, lists, _cols(SC.PICK), max_entries=max(SC.SHORT))
    b, _ = _run(plain, lists, _cols(SC.PICK), max_entries=max(SC.SHORT))
    assert np.array_equal(_bits(a), _bits(b))


def test_out_of_range_entries_are_clamped_and_flagged():
    """the clamp, not a fault: a clamped row is valid memory of the store"""
    grid = GRIDS[0]
    store = _store(grid, None)
    x = _decoded(grid, None)
    T = store.shape[0]
    base = [[4, 7], [5]]
    got, flag = _run(store, base, [1], max_entries=2)
    assert flag == 0
    _assert_same(got, SO.slot_climatology(x, base, [1], SC.DRY))
    got, flag = _run(store, base, [1], rows=[4, T + 5, -3], max_entries=2)                   # rows beyond both ends
    assert flag == 1
    _assert_same(got, SO.slot_climatology(x, [[4, T - 1], [0]], [1], SC.DRY))
    ten = [[3, 30, 300, 11, 12, 13, 14, 15, 500, 501], [9]]                                  # longer than max_entries
    got, flag = _run(store, ten, [1, 2], max_entries=8)
    assert flag == 1
    _assert_same(got, SO.slot_climatology(x, [ten[0][:8], [9]], [1, 2], SC.DRY))


def test_a_negative_zero_dry_threshold_is_zero():
    """-0.0 as the threshold compares as +0.0 does: nothing finite and non-negative is below it"""
    store = _store(GRIDS[0], None)
    lists = SC.hand_lists(store.shape[0], (61,), 34)
    a, _ = _run(store, lists, [1], dry=-0.0, max_entries=61)
    b, _ = _run(store, lists, [1], dry=0.0, max_entries=61)
    assert np.array_equal(_bits(a), _bits(b))
    _assert_same(a, SO.slot_climatology(_decoded(GRIDS[0], None), lists, [1], 0.0))
    assert bool((a[0][np.isfinite(a[0])] == 0).all())


# ---------------------------------------------------------------------------------- plans
def _oracle_lists(key):
    kw = dict(PLANS[key])
    if "start" in kw:
        kw["start"] = np.datetime64(kw["start"] + "T00:00:00")
        kw["end"] = np.datetime64(kw["end"] + "T23:59:59")
    return SO.slot_lists(_times(), **kw)[0]


@pytest.mark.parametrize("key,packing", [("w1", None), ("w61", None), ("w61", "u16")])
def test_build_seeps_equals_the_oracle(key, packing):
    from paradis_model_amd import climatology
    grid = GRIDS[0]
    H, W = grid
    store = _store(grid, packing)
    plan = climatology.ClimPlan(store.times_us, **PLANS[key])
    names = ["total_precipitation_6hr", "total_precipitation_24hr"]
    sc = climatology.build_seeps(store, plan, names, SC.DRY)
    assert isinstance(sc, climatology.SeepsClimatology) and tuple(sc.data.shape) == (2, plan.n_slots, 2, H, W)
    assert sc.data.dtype == torch.float32 and sc.data.device == store.device and sc.names == names and sc.plan is plan
    assert sc.dry_threshold == SC.DRY and sc.wet_level == 2.0 / 3.0 and sc.min_count == 1
    assert sc.p1.data_ptr() == sc.data[0].data_ptr() and sc.threshold.data_ptr() == sc.data[1].data_ptr()
    want = SO.slot_climatology(_decoded(grid, packing), _oracle_lists(key), _cols(names), SC.DRY)
    _assert_same(sc.data.cpu().numpy(), want, f"{key} {packing}")
    if key == "w1":
        k = plan.days.index(366) * len(plan.hours)
        assert plan.entries[k] == 0 and bool(torch.isnan(sc.data[:, k]).all())       # the slot start / end emptied
        idx = sc.index(store.times_us.numpy()[[0, 5]])
        assert idx.dtype == torch.int32 and idx.device == store.device
        assert idx.tolist() == plan.slot_of(store.times_us.numpy()[[0, 5]]).tolist()
    else:
        assert plan.entries.max() > 100
    again = climatology.build_seeps(store, plan, names, SC.DRY, wet_level=0.5, min_count=2)
    assert again.wet_level == 0.5 and again.min_count == 2
    both = ~torch.isnan(again.data[0])
    assert torch.equal(again.data[0][both], sc.data[0][both])                        # p1 does not move with the level
