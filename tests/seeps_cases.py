"""The test data of the SEEPS tests (tests/test_seeps_cpu.py, tests/test_hip_seeps_clim.py, tests/test_hip_seeps.py):
numpy only, needs no GPU.  Test infrastructure; reads nothing outside the repository.

Precipitation: ``|N(0, 1)| * 1e-3``, set to 0.0 with a probability that ramps linearly from 0 at the first column to 1
at the last, a few of the zeros -0.0; the first columns get +1e-3 on every value, so they are always wet and ``p1 = 0``;
``DRY = 0.25e-3``.  About a fifth of the values that stay are below ``DRY`` (P(|z| < 0.25) = 0.197), so a column whose
zero probability is r has p1 ~ r + 0.197 (1 - r): with the bounds (0.1, 0.85) the columns up to r ~ 0.81 are inside, the
last column is all dry, the ones before it have p1 > p_hi, and only the always-wet columns have p1 < p_lo.  Two
always-wet columns of a row of 7 or 10 cells would leave 3 of 7 / 5 or 6 of 10 columns inside - at or under the 50 % the
designs must keep -, so rows of fewer than 16 cells get ONE always-wet column and wider rows two.  tests/test_seeps_cpu.py
asserts, through the oracle, that every design below has cells of each class and at least half of its cells inside."""
import functools

import numpy as np

from tests import seeps_oracle as SO

DRY = float(np.float32(0.25e-3))
P_LO, P_HI = 0.1, 0.85
CLIM_GRIDS = [(6, 10), (5, 7), (7, 20)]
DESIGN_LISTS = (9, 61, 257)                        # the list lengths whose class conditions the CPU test asserts


def wet_columns(W):
    return 2 if W >= 16 else 1


def precipitation(T, H, W, seed):
    """float32 [T, H, W] by the design of the module docstring; read-only"""
    rng = np.random.default_rng(seed)
    p = (np.abs(rng.standard_normal((T, H, W))) * 1e-3).astype(np.float32)
    ramp = np.arange(W, dtype=np.float64) / float(max(W - 1, 1))
    u = rng.random((T, H, W))
    zero = u < ramp
    p[zero] = 0.0
    p[zero & (rng.random((T, H, W)) < 0.05)] = -0.0
    p[:, :, :wet_columns(W)] += np.float32(1e-3)
    p.setflags(write=False)
    return p


# ---------------------------------------------------------------------------------- the climatology's stores
FEATURES = ["temperature_h850", "total_precipitation_6hr", "total_precipitation_24hr"]
PICK = ["total_precipitation_6hr", "total_precipitation_24hr", "temperature_h850"]
SHORT = [0, 1, 2, 3, 9, 61, 128, 129, 257]         # hand-made lists; 257 entries need the 128 KiB tile
ONE_WET_ROW = 7                                    # the store row every non-empty hand-made list begins with
CELL_ALL_AT_DRY = (2, 3)                           # every value == DRY: strictly nothing is below it, all wet
CELL_ONE_WET = (3, 4)                              # 0.0 everywhere but in row ONE_WET_ROW


@functools.lru_cache(maxsize=None)
def store_data(grid, T=857):
    """float32 [T, 3, H, W]: the features above; pixel (0, 1) NaN in every third row, pixel (H - 1, W - 2) NaN in every
    row, pixel (1, 0) +Inf in every fifth row (tests/test_hip_quantile.py's), and the two planted precipitation cells"""
    H, W = grid
    seed = 4100 + 10 * H + W
    rng = np.random.default_rng(seed)
    x = np.empty((T, len(FEATURES), H, W), np.float32)
    x[:, 0] = (250.0 + 15.0 * rng.standard_normal((T, H, W))).astype(np.float32)
    x[:, 1] = precipitation(T, H, W, seed + 1)
    x[:, 2] = precipitation(T, H, W, seed + 2)
    for j in (1, 2):
        x[:, j, CELL_ALL_AT_DRY[0], CELL_ALL_AT_DRY[1]] = np.float32(DRY)
        x[:, j, CELL_ONE_WET[0], CELL_ONE_WET[1]] = 0.0
        x[ONE_WET_ROW, j, CELL_ONE_WET[0], CELL_ONE_WET[1]] = np.float32(2e-3)
    x[::3, :, 0, 1] = np.nan
    x[:, :, H - 1, W - 2] = np.nan
    x[::5, :, 1, 0] = np.inf
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def hand_lists(T, lengths, seed):
    """per slot a tuple of rows in no order: ONE_WET_ROW first, the rest drawn at random without it"""
    rng = np.random.default_rng(seed)
    others = np.array([r for r in range(T) if r != ONE_WET_ROW])
    return tuple(tuple([ONE_WET_ROW] + [int(r) for r in rng.choice(others, n - 1, replace=False)]) if n else ()
                 for n in lengths)


# ---------------------------------------------------------------------------------- the update's designs
# name -> (B, H, W, K, Cs); the state has C = Cs + 1 channels, the scored ones are the state's LAST Cs in reverse order
UPDATE_SHAPES = {
    "small": (3, 5, 10, 3, 2),        # scalar path (W % 4 != 0), a partial walk, fewer rows than four waves' second turn
    "groups": (2, 33, 260, 1, 1),     # vector path, two walks per row, the second holding one quad; row groups of 31 + 2
    "odd": (2, 6, 7, 1, 1),           # odd width
    "walks": (1, 2, 512, 1, 1),       # two full walks, no tail
}
N_CLIM = 40                           # values per cell behind an update design's climatology
EXACT_ROW = {"small": 4, "groups": 32, "odd": 5, "walks": 1}      # the row with exactly one valid cell


@functools.lru_cache(maxsize=None)
def update_climatology(name):
    """float32 [2, K, Cs, H, W] through the oracle from N_CLIM ramp fields per (slot, channel); read-only"""
    B, H, W, K, Cs = UPDATE_SHAPES[name]
    seed = 5200 + 7 * H + W
    x = np.stack([precipitation(N_CLIM, H, W, seed + j) for j in range(K * Cs)], axis=1)      # [N, K Cs, H, W]
    data = SO.slot_climatology(x, [list(range(N_CLIM))], list(range(K * Cs)), DRY)            # [2, 1, K Cs, H, W]
    data = np.ascontiguousarray(data.reshape(2, K, Cs, H, W))
    data.setflags(write=False)
    return data


def _value_of(category, thr):
    """a float32 value of the category: 0.0, the midpoint of [DRY, thr], 2 thr"""
    thr = np.float32(thr)
    return np.float32(0.0) if category == 0 else (np.float32(0.5) * (np.float32(DRY) + thr) if category == 1
                                                  else np.float32(2.0) * thr)


@functools.lru_cache(maxsize=None)
def update_case(name, want=0):
    """``(fc, truth, data, clim_index, chan, C)``: float32 states [B, C, H, W] drawn by the same ramp design (so every
    category occurs in both), with planted ties ``f == thr`` and ``o == dry`` and a NaN in each of the four inputs in
    turn, and row EXACT_ROW[name] emptied (NaN forecasts) in every sample and channel but for ONE cell of sample 0,
    whose truth has category ``want`` and whose forecast category ``(want + 1) % 3``: that row's sums are one cell's
    ``s``.  Read-only."""
    B, H, W, K, Cs = UPDATE_SHAPES[name]
    C = Cs + 1
    seed = 6300 + 7 * H + W
    data = update_climatology(name).copy()
    fc = np.empty((B, C, H, W), np.float32)
    tr = np.empty((B, C, H, W), np.float32)
    for c in range(C):
        fc[:, c] = precipitation(B, H, W, seed + 2 * c)
        tr[:, c] = precipitation(B, H, W, seed + 2 * c + 1)
    chan = [C - 1 - cs for cs in range(Cs)]
    clim_index = np.array([(b * 2) % K for b in range(B)], np.int32)
    inside = SO.classes(data)["inside"]                                   # [K, Cs, H, W]
    k0, c0 = int(clim_index[0]), chan[0]
    # ties and NaNs of sample 0, channel 0, at cells inside the bounds: rows 0 and 1 (row 0 alone where row 1 is EXACT_ROW)
    ha, hb = 0, (1 if EXACT_ROW[name] != 1 else 0)
    wa, wb = np.flatnonzero(inside[k0, 0, ha])[:3], np.flatnonzero(inside[k0, 0, hb])[-3:]
    assert wa.size == 3 and wb.size == 3 and (ha != hb or wa[-1] < wb[0]), name
    fc[0, c0, ha, wa[0]] = data[1, k0, 0, ha, wa[0]]                       # f == thr: heavy
    tr[0, c0, ha, wa[1]] = np.float32(DRY)                                # o == dry: not dry
    fc[0, c0, ha, wa[2]] = np.nan
    tr[0, c0, hb, wb[0]] = np.nan
    data[0, k0, 0, hb, wb[1]] = np.nan                                    # p1
    data[1, k0, 0, hb, wb[2]] = np.nan                                    # thr
    h = EXACT_ROW[name]
    for cs in range(Cs):
        fc[:, chan[cs], h, :] = np.nan
        w = int(np.flatnonzero(inside[k0, cs, h])[0])
        thr = data[1, k0, cs, h, w]
        fc[0, chan[cs], h, w] = _value_of((want + 1) % 3, thr)
        tr[0, chan[cs], h, w] = _value_of(want, thr)
    for a in (fc, tr, data, clim_index):
        a.setflags(write=False)
    return fc, tr, data, clim_index, chan, C
