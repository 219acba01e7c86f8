"""GPU: the quantile climatology (paradis_model_amd/climatology.py ``clim_quantile`` / ``build_quantiles``,
csrc/quantile.hip ``paradis_clim_quantile`` / ``paradis_clim_quantile_packed``) against the numpy restatement of
tests/quantile_oracle.py, and its use as per-cell thresholds of ``EventTable`` and ``ProbabilityTable``.

Stores as in tests/test_hip_clim.py: F = 9 features over the 857 times of ``clim_oracle.case_times``, float32 and
``packing="u16"``, the oracle fed ``store.rows(0, T).cpu()``; pixel (0, 1) NaN in every third row, pixel (H - 1, W - 2)
NaN in every row, pixel (1, 0) +Inf in every fifth row.  The precipitation is exactly 0.0 in about 70 % of the cells and
-0.0 in a few.  A second store of three features on the (6, 10) grid has T = 2100 rows, for the long lists.

Grids sit on the kernel's edges; with lists of 129 to 512 entries a workgroup owns ``paradis_clim_quantile_cells()`` =
64 adjacent cells of a plane:
  (6, 10)   P = 60: vector path, one partial tile (P < cells)
  (5, 7)    P = 35: odd, scalar path
  (7, 20)   P = 140: two full tiles and a tail of 12 cells
Longer lists get fewer cells per workgroup - 32 up to 1024 entries, 16 up to 2048, 8 up to 4096 -, which the long
store's P = 60 divides in none of the three cases.  Shorter lists get more - 128 up to 128 entries, 256 up to 64, 512 up
to 32, 1024 up to 16 -: (33, 64), P = 2112, is whole tiles and a tail of 64 cells for each of them, (7, 20) a 128-cell
tile and a tail of 12, (5, 7) the scalar path under a tile wider than the plane.

Hand-made CSR lists (rows drawn at random, not sorted) of 0 (NaN), 1, 2, 3, 8, 9, 127, 128, 129, 255, 256, 257 entries
under the 64-cell tile and, up to 128, under the wide tile of their own length as well; 600 and 1024, 1025, 2049 and
4096 entries, each class with a 5-entry list beside the long ones.

Bound: none.  The kernel sorts exactly, the rest is IEEE double multiply, subtract, add, floor and one rounding,
uncontracted on both sides: every output equals the oracle's bit for bit (as uint32), NaN exactly where it has NaN."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import clim_oracle as CO
from tests import forecast_oracle as FO
from tests import quantile_oracle as QO

pytestmark = pytest.mark.gpu

GRIDS = [(6, 10), (5, 7), (7, 20)]
LONG_GRID = (6, 10)
LEVELS = [0.0, 0.05, 1.0 / 3.0, 0.5, 0.95, 1.0]
PLEVELS = [500, 850]
FEATURES = ["wind_x_h500", "temperature_h500", "wind_y_h500", "total_precipitation_6hr", "wind_z_h500",
            "temperature_h850", "wind_x_h850", "wind_y_h850", "wind_z_h850"]
NAMES = ["temperature_h500", "temperature_h850", "wind_x_h500", "wind_x_h850", "wind_y_h500", "wind_y_h850",
         "wind_z_h500", "wind_z_h850", "total_precipitation_6hr"]
LONG_FEATURES = ["temperature_h850", "wind_x_h850", "total_precipitation_6hr"]
PICK = ["total_precipitation_6hr", "temperature_h850", "wind_x_h500"]          # the channels of the hand-made lists
PLANS = {
    "w1": dict(start="2019-12-01", end="2020-12-30", window_days=1),
    "w61": dict(days=[1, 60, 200, 366], window_days=61),
}
SHORT = [0, 1, 2, 3, 8, 9, 127, 128, 129, 255, 256, 257]
# max_entries -> list lengths: one launch per tile class above 512 entries
LONG = {1024: [600, 5, 1024], 1025: [1025, 5], 2049: [5, 2049], 4096: [4096, 5, 2100]}
LONG_CELLS = {1024: 32, 1025: 16, 2049: 8, 4096: 8}
# the wide tiles of short lists: max_entries -> list lengths
WIDE = {8: [0, 1, 2, 3, 8, 5], 16: [9, 16, 4], 32: [17, 32, 5], 64: [33, 64, 5], 128: [65, 127, 128, 5]}
WIDE_CELLS = {8: 1024, 16: 1024, 32: 512, 64: 256, 128: 128}
WIDE_GRID = (33, 64)


def test_shapes_sit_on_the_kernel_edges():
    from paradis_model_amd import _lib
    cells = _lib.lib.paradis_clim_quantile_cells
    assert cells(max(SHORT)) == 64 and cells(129) == 64 and cells(512) == 64
    assert {n: cells(n) for n in WIDE} == WIDE_CELLS and cells(1) == 1024 and cells(16) == 1024 and cells(17) == 512
    Pw = WIDE_GRID[0] * WIDE_GRID[1]
    for c in WIDE_CELLS.values():
        assert Pw > 2 * c and Pw % c == 64 and 35 < c
    assert 140 > 128 and 140 % 128 == 12
    assert [h * w for h, w in GRIDS] == [60, 35, 140]
    P = [h * w for h, w in GRIDS]
    assert P[0] < 64 and P[0] % 4 == 0 and P[1] % 4 != 0 and P[2] > 2 * 64 and P[2] % 64 == 12 and P[2] % 4 == 0
    assert {n: cells(n) for n in LONG} == LONG_CELLS
    for c in LONG_CELLS.values():
        assert 60 > c and 60 % c != 0
    assert _lib.lib.paradis_clim_quantile_max_entries() == 4096


# ---------------------------------------------------------------------------------- stores
@functools.lru_cache(maxsize=None)
def _times(T=None):
    if T is None:
        t = CO.case_times()
    else:
        t = (np.datetime64("2015-01-01T00", "h") + 6 * np.arange(T).astype("timedelta64[h]")).astype("datetime64[us]")
    t.setflags(write=False)
    return t


def _grid(H, W):
    return FO.grid_deg(H, W, False)


def _fill(x, features, g):
    T, F, H, W = x.shape
    for j, f in enumerate(features):
        b = FO.base_name(f)
        if b == "temperature":
            x[:, j] = 250.0 + 15.0 * x[:, j]
        elif b == "total_precipitation_6hr":
            u = torch.rand(T, H, W, generator=g)
            p = x[:, j].abs() * 1e-3
            p[u < 0.7] = 0.0
            p[u < 0.03] = -0.0
            x[:, j] = p
        else:
            x[:, j] *= 10.0
    x[::3, :, 0, 1] = float("nan")
    x[:, :, H - 1, W - 2] = float("nan")
    x[::5, :, 1, 0] = float("inf")
    return x


@functools.lru_cache(maxsize=None)
def _raw(grid, long=False):
    H, W = grid
    feats = LONG_FEATURES if long else FEATURES
    T = 2100 if long else _times().size
    g = torch.Generator().manual_seed(900 + 10 * int(long) + (GRIDS.index(grid) if grid in GRIDS else 7))
    return _fill(torch.randn(T, len(feats), H, W, generator=g), feats, g)


def _make_store(data, times, feats, grid, packing):
    from paradis_model_amd.dataset import DeviceStore
    H, W = grid
    lat, lon = _grid(H, W)
    stats = {k: np.ones(len(feats), np.float32) for k in ("mean", "std", "min", "max")}
    return DeviceStore(data, times, feats, stats, lat, lon, np.zeros((H, W, 1), np.float32), toa_mean=0.0, toa_std=1.0,
                       device="cuda", packing=packing)


@functools.lru_cache(maxsize=None)
def _store(grid, packing, long=False):
    return _make_store(_raw(grid, long).numpy(), _times(2100 if long else None), LONG_FEATURES if long else FEATURES,
                       grid, packing)


@functools.lru_cache(maxsize=None)
def _decoded(grid, packing, long=False):
    """what the store holds, as float32 numpy: the oracle's input, read once and never written"""
    store = _store(grid, packing, long)
    x = store.rows(0, store.shape[0]).cpu().numpy()
    x.setflags(write=False)
    return x


def _cols(feats, names):
    return [feats.index(n) for n in names]


@functools.lru_cache(maxsize=None)
def _hand_lists(T, lengths, seed):
    """per slot a tuple of rows, drawn at random (with repeats only where a list is longer than the store)"""
    rng = np.random.default_rng(seed)
    return tuple(tuple(int(r) for r in rng.choice(T, n, replace=n > T)) for n in lengths)


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    return ptr, np.array([r for l in lists for r in l], np.int64)


def _run(store, lists, cols, levels=LEVELS, ptr=None, rows=None, **kw):
    from paradis_model_amd.climatology import clim_quantile
    dev = store.device
    p, r = _csr(lists)
    ptr = p if ptr is None else np.asarray(ptr, np.int64)
    rows = r if rows is None else np.asarray(rows, np.int64)
    out, flag = clim_quantile(store, torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev),
                              torch.tensor(cols, dtype=torch.int32, device=dev), levels, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(flag.item())


@functools.lru_cache(maxsize=None)
def _want_short(grid, packing):
    x = _decoded(grid, packing)
    want = QO.slot_quantiles(x, _hand_lists(x.shape[0], tuple(SHORT), 31), _cols(FEATURES, PICK), LEVELS)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _want_long(packing, max_entries):
    x = _decoded(LONG_GRID, packing, True)
    want = QO.slot_quantiles(x, _hand_lists(x.shape[0], tuple(LONG[max_entries]), 32), [0, 1, 2], LEVELS)
    want.setflags(write=False)
    return want


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    """bit for bit as uint32, NaN exactly where the oracle has NaN (the oracle's NaN and the kernel's are the same
    quiet NaN only by luck: NaN cells are compared as NaN)"""
    assert got.shape == want.shape and got.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"


# ---------------------------------------------------------------------------------- hand-made lists
@pytest.mark.parametrize("packing", [None, "u16"])
@pytest.mark.parametrize("grid", GRIDS)
def test_list_lengths_bit_for_bit(grid, packing):
    store = _store(grid, packing)
    T = store.shape[0]
    H, W = grid
    lists = _hand_lists(T, tuple(SHORT), 31)
    cols = _cols(FEATURES, PICK)
    got, flag = _run(store, lists, cols, max_entries=max(SHORT))
    want = _want_short(grid, packing)
    assert flag == 0 and got.shape == (len(LEVELS), len(SHORT), len(PICK), H, W)
    _assert_same(got, want, f"{grid} {packing}")
    assert bool(np.isnan(got[:, 0]).all())                              # the empty list
    assert bool(np.isnan(got[:, :, :, H - 1, W - 2]).all())             # the all-missing pixel
    assert bool(np.isfinite(got[:, 1:, :, 2, 3]).all())
    x = _decoded(grid, packing)
    kept = np.stack([np.isfinite(x[list(l)][:, cols]).sum(axis=0) if l else np.zeros((len(cols), H, W), np.int64)
                     for l in lists])                                   # [K, C, H, W]
    assert np.array_equal(np.isnan(got[0]), kept == 0)
    # the levels 0 and 1 are the smallest and the largest value kept; -0.0 never comes out
    k = SHORT.index(129)
    sub = np.where(np.isfinite(x[list(lists[k])][:, cols]), x[list(lists[k])][:, cols], np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # all-NaN cells
        assert np.array_equal(got[0, k], np.nanmin(sub, axis=0), equal_nan=True)
        assert np.array_equal(got[-1, k], np.nanmax(sub, axis=0), equal_nan=True)
    assert not bool((_bits(got) == 0x80000000).any())
    if packing is None:
        assert int((got[0, :, 0] == 0).sum()) > 0                       # the dry cells' minimum
    # min_count = 3 turns cells with 1 or 2 values kept into NaN and changes nothing else
    got3, flag = _run(store, lists, cols, max_entries=max(SHORT), min_count=3)
    few = np.broadcast_to((kept < 3)[None], got.shape)
    assert flag == 0 and bool(np.isnan(got3[few]).all()) and np.array_equal(_bits(got3[~few]), _bits(got[~few]))
    assert int(((kept > 0) & (kept < 3)).sum()) > 0
    # two runs: equal bit for bit
    again, _ = _run(store, lists, cols, max_entries=max(SHORT))
    assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("packing", [None, "u16"])
def test_short_lists_under_the_longest_tile(packing):
    """the default max_entries (4096: 8 cells per workgroup, 512 KiB of sentinels never sorted) gives the same bits"""
    store = _store(GRIDS[0], packing)
    lists = _hand_lists(store.shape[0], tuple(SHORT), 31)
    got, flag = _run(store, lists, _cols(FEATURES, PICK))
    assert flag == 0
    _assert_same(got, _want_short(GRIDS[0], packing))


@functools.lru_cache(maxsize=None)
def _want_wide(grid, packing, max_entries):
    x = _decoded(grid, packing)
    want = QO.slot_quantiles(x, _hand_lists(x.shape[0], tuple(WIDE[max_entries]), 33), _cols(FEATURES, PICK[:2]), LEVELS)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("grid,packing", [(WIDE_GRID, None), (WIDE_GRID, "u16"), (GRIDS[1], None), (GRIDS[2], "u16")])
def test_short_lists_under_their_wide_tiles(grid, packing):
    """lists up to 128 entries under the tile of their own length: 1024, 512, 256 and 128 cells per workgroup"""
    store = _store(grid, packing)
    for max_entries in WIDE:
        lists = _hand_lists(store.shape[0], tuple(WIDE[max_entries]), 33)
        got, flag = _run(store, lists, _cols(FEATURES, PICK[:2]), max_entries=max_entries)
        assert flag == 0
        _assert_same(got, _want_wide(grid, packing, max_entries), f"{grid} {packing} {max_entries}")
        again, _ = _run(store, lists, _cols(FEATURES, PICK[:2]), max_entries=max_entries)
        assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("max_entries", list(LONG))
@pytest.mark.parametrize("packing", [None, "u16"])
def test_long_lists_bit_for_bit(packing, max_entries):
    store = _store(LONG_GRID, packing, True)
    lists = _hand_lists(store.shape[0], tuple(LONG[max_entries]), 32)
    got, flag = _run(store, lists, [0, 1, 2], max_entries=max_entries)
    assert flag == 0
    _assert_same(got, _want_long(packing, max_entries), f"{packing} {max_entries}")
    assert bool(np.isfinite(got[:, :, :, 2, 3]).all())


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
def test_packed_store_equals_the_float32_store_of_its_decoded_rows(grid):
    packed = _store(grid, "u16")
    plain = _make_store(_decoded(grid, "u16").copy(), _times(), FEATURES, grid, None)
    lists = _hand_lists(packed.shape[0], tuple(SHORT), 31)
    cols = _cols(FEATURES, PICK)
    a, _ = _run(packed, lists, cols, max_entries=max(SHORT))
    b, _ = _run(plain, lists, cols, max_entries=max(SHORT))
    assert np.array_equal(_bits(a), _bits(b))


def test_out_of_range_entries_are_clamped_and_flagged():
    """the clamp, not a fault: a clamped row, column or list is valid memory of the store and of the lists"""
    grid = GRIDS[0]
    store = _store(grid, None)
    x = _decoded(grid, None)
    T, F = store.shape[:2]
    levels = [0.0, 0.5, 1.0]

    def want(lists, cols):
        return QO.slot_quantiles(x, lists, cols, levels)

    base = [[4, 7], [5]]
    got, flag = _run(store, base, [0, 2], levels, max_entries=2)
    assert flag == 0
    _assert_same(got, want(base, [0, 2]))
    got, flag = _run(store, base, [0, 2], levels, rows=[4, T + 5, -3], max_entries=2)       # rows beyond both ends
    assert flag == 1
    _assert_same(got, want([[4, T - 1], [0]], [0, 2]))
    got, flag = _run(store, base, [F + 2, -1], levels, max_entries=2)                        # columns beyond both ends
    assert flag == 1
    _assert_same(got, want(base, [F - 1, 0]))
    got, flag = _run(store, base, [0], levels, ptr=[0, 2, 9], max_entries=2)                 # a list bound beyond N
    assert flag == 1
    _assert_same(got, want(base, [0]))
    ten = [[3, 30, 300, 11, 12, 13, 14, 15, 500, 501], [9]]                                  # longer than max_entries
    got, flag = _run(store, ten, [0, 3], levels, max_entries=8)
    assert flag == 1
    _assert_same(got, want([ten[0][:8], [9]], [0, 3]))
    got, flag = _run(store, ten, [0, 3], levels, max_entries=10)
    assert flag == 0
    _assert_same(got, want(ten, [0, 3]))


# ---------------------------------------------------------------------------------- plans
def _oracle_lists(key):
    kw = dict(PLANS[key])
    if "start" in kw:
        kw["start"] = np.datetime64(kw["start"] + "T00:00:00")
        kw["end"] = np.datetime64(kw["end"] + "T23:59:59")
    return QO.slot_lists(_times(), **kw)[0]


def _plan(store, key):
    from paradis_model_amd.climatology import ClimPlan
    return ClimPlan(store.times_us, **PLANS[key])


@pytest.mark.parametrize("key,packing", [("w1", None), ("w61", None), ("w61", "u16")])
def test_build_quantiles_equals_the_oracle(key, packing):
    from paradis_model_amd import climatology
    grid = GRIDS[0]
    H, W = grid
    store = _store(grid, packing)
    plan = _plan(store, key)
    names = ["total_precipitation_6hr", "temperature_h850"]
    levels = [0.05, 0.5, 0.95]
    qc = climatology.build_quantiles(store, plan, levels, names=names)
    assert tuple(qc.data.shape) == (3, plan.n_slots, 2, H, W) and qc.data.dtype == torch.float32
    assert qc.data.device == store.device and qc.names == names and qc.levels == levels and qc.plan is plan
    want = QO.slot_quantiles(_decoded(grid, packing), _oracle_lists(key), _cols(FEATURES, names), levels)
    _assert_same(qc.data.cpu().numpy(), want, f"{key} {packing}")
    if key == "w1":
        k = plan.days.index(366) * len(plan.hours)
        assert plan.entries[k] == 0 and bool(torch.isnan(qc.data[:, k]).all())       # the slot start / end emptied
    else:
        assert plan.entries.max() > 100
    assert torch.equal(qc.level(0.5), qc.data[1])
    again = climatology.build_quantiles(store, plan, levels, names=names, min_count=2)
    assert again.min_count == 2 and bool((torch.isnan(again.data) | (again.data == qc.data)).all())


# ---------------------------------------------------------------------------------- per-cell thresholds, end to end
@functools.lru_cache(maxsize=None)
def _thresholds():
    """(field [K, 9, H, W] on the device, its numpy copy, the slots of B = 3 samples, forecast and truth numpy
    [3, 9, H, W] and a 4-member ensemble [12, 9, H, W]): q90 of the precipitation, q10 of temperature_h850"""
    from paradis_model_amd import climatology
    grid = GRIDS[0]
    store = _store(grid, None)
    plan = _plan(store, "w61")
    qc = climatology.build_quantiles(store, plan, [0.1, 0.9], names=["total_precipitation_6hr", "temperature_h850"])
    field = qc.field(NAMES, {"total_precipitation_6hr": 0.9, "temperature_h850": 0.1})
    q = field.cpu().numpy()
    slots = np.array([0, 3, 5], np.int32)
    x = _decoded(grid, None)[:, _cols(FEATURES, NAMES)]
    fc, tr, ens = x[[10, 200, 411]].copy(), x[[12, 202, 415]].copy(), x[20:32].copy()
    cp, ct = NAMES.index("total_precipitation_6hr"), NAMES.index("temperature_h850")
    qb = q[slots]
    up, down = np.float32(np.inf), np.float32(-np.inf)
    for c in (cp, ct):                                  # ties and their neighbours one ulp away
        fc[:, c, 2], tr[:, c, 2] = qb[:, c, 2], np.nextafter(qb[:, c, 2], up)
        fc[:, c, 3], tr[:, c, 3] = np.nextafter(qb[:, c, 3], down), qb[:, c, 3]
        ens[0::4, c, 2], ens[1::4, c, 2] = qb[:, c, 2], np.nextafter(qb[:, c, 2], down)
        ens[2::4, c, 3] = np.nextafter(qb[:, c, 3], up)
    return field, q, slots, fc, tr, ens


def test_event_table_counts_x_against_its_cell_quantile():
    from paradis_model_amd.climatology import quantile_event
    from paradis_model_amd.events import EventTable
    field, q, slots, fc, tr, _ = _thresholds()
    H, W = GRIDS[0]
    lat, _ = _grid(H, W)
    events = {"wet": quantile_event("total_precipitation_6hr"), "cold": quantile_event("temperature_h850", "le")}
    table = EventTable(NAMES, lat, 1, events, climatology=field)
    table.update(0, torch.from_numpy(fc).cuda(), torch.from_numpy(tr).cuda(), torch.from_numpy(slots).cuda())
    cnt = table.counts()
    qb = q[slots]
    for s, (name, op) in enumerate((("total_precipitation_6hr", np.greater_equal), ("temperature_h850", np.less_equal))):
        c = NAMES.index(name)
        f, t, th = fc[:, c], tr[:, c], qb[:, c]
        valid = np.isfinite(f) & np.isfinite(t) & np.isfinite(th)
        with np.errstate(invalid="ignore"):
            F, O = valid & op(f, th), valid & op(t, th)                   # no subtraction
        assert np.array_equal(cnt["valid"][0, s], valid.sum(axis=(0, 2)))
        assert np.array_equal(cnt["forecast_yes"][0, s, :, 0], F.sum(axis=(0, 2)))
        assert np.array_equal(cnt["observed_yes"][0, s, :, 0], O.sum(axis=(0, 2)))
        assert np.array_equal(cnt["both"][0, s, :, 0], (F & O).sum(axis=(0, 2)))
        assert 0 < int(F.sum()) < int(valid.sum()) and int(valid.sum()) < valid.size
        assert int(F[:, 2].sum()) == int(valid[:, 2].sum()) > 0           # x == q is the event, either direction
    assert int(cnt["n_samples"][0]) == 3


def test_probability_table_counts_members_against_the_cell_quantile():
    from paradis_model_amd.climatology import quantile_event
    from paradis_model_amd.probability import ProbabilityTable
    field, q, slots, _, tr, ens = _thresholds()
    H, W = GRIDS[0]
    M = 4
    lat, _ = _grid(H, W)
    events = {"wet": quantile_event("total_precipitation_6hr"), "cold": quantile_event("temperature_h850", "le")}
    table = ProbabilityTable(NAMES, lat, 1, events, M, climatology=field)
    table.update(0, torch.from_numpy(ens).cuda(), torch.from_numpy(tr).cuda(), torch.from_numpy(slots).cuda())
    cnt = table.counts()
    qb = q[slots]
    for s, (name, op) in enumerate((("total_precipitation_6hr", np.greater_equal), ("temperature_h850", np.less_equal))):
        c = NAMES.index(name)
        t, th = tr[:, c], qb[:, c]
        valid = np.isfinite(t) & np.isfinite(th)
        k = np.zeros(t.shape, np.int64)
        with np.errstate(invalid="ignore"):
            o = op(t, th).astype(np.int64)
            for i in range(M):
                m = ens[i::M, c]
                valid &= np.isfinite(m)
                k += op(m, th)
        joint = np.zeros((H, 2, M + 1), np.int64)
        for g, h, w in zip(*np.nonzero(valid)):
            joint[h, o[g, h, w], k[g, h, w]] += 1
        assert np.array_equal(cnt["valid"][0, s], valid.sum(axis=(0, 2)))
        assert np.array_equal(cnt["joint"][0, s, :, 0], joint)
        assert int(joint[:, 1].sum()) > 0 and int(joint[:, 0].sum()) > 0
    assert int(cnt["n_samples"][0]) == 3
