"""GPU: the verification climatology (paradis_model_amd/climatology.py ``build``, csrc/climatology.hip
``paradis_clim_mean`` / ``paradis_clim_mean_packed`` / ``paradis_spherical_winds_inplace``) against the numpy fp64
restatement of tests/clim_oracle.py.

Stores: F = 9 features - temperature, wind_x, wind_y, wind_z at two levels and total_precipitation_6hr, in an order that
is NOT the climatology's channel order - over the 857 times of ``clim_oracle.case_times`` (2019-12-01 .. 2021-02-01, 12 h),
float32 and ``packing="u16"`` (log-packed precipitation).  The oracle is fed ``store.rows(0, T).cpu()``, so both see the
same decoded values.  Winds are O(10) m/s and temperatures 250 +- 15 K, so every rotated component is of the size of its
inputs.  Pixel (0, 1) is NaN in every third row (it loses some entries of a slot), pixel (H - 1, W - 2) in every row (it
loses all of them), pixel (1, 0) is +Inf in every fifth row.

Grids sit on the kernel's edges; a workgroup owns ``paradis_clim_mean_chunk()`` = 1024 values of a plane:
  (6, 10)   P = 60: vector path, one partial chunk
  (5, 7)    P = 35: odd, scalar path
  (33, 64)  P = 2112: two full chunks and a tail of 64 values
Lists: window 1 between ``start`` and ``end`` (one entry per slot, slot 366 empty), window 61 on a subset of days (lists
of 100 and more entries: longer than the kernel's 8 rows in flight, and not a multiple of it), window 5 with gaussian
weights.

Bounds.  ``winds=False``: the inputs are identical and S, Wt are double sums in list order on both sides, so only the
last rounding can differ: every finite output within 1 float32 ulp of the oracle's fp64 mean rounded to float32, NaN
exactly where the oracle has NaN.  With the ``PostSpec``: non-wind channels bit for bit the ``winds=False`` run, wind
channels max|x - ref| / max|ref| <= 1e-6 per channel, the bound tests/test_hip_forecast.py holds post.hip's winds to."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import clim_oracle as CO
from tests import forecast_oracle as FO

pytestmark = pytest.mark.gpu

CHUNK = 1024
GRIDS = [(6, 10), (5, 7), (33, 64)]
LEVELS = [500, 850]
FEATURES = ["wind_x_h500", "temperature_h500", "wind_y_h500", "total_precipitation_6hr", "wind_z_h500",
            "temperature_h850", "wind_x_h850", "wind_y_h850", "wind_z_h850"]
NAMES = ["temperature_h500", "temperature_h850", "wind_x_h500", "wind_x_h850", "wind_y_h500", "wind_y_h850",
         "wind_z_h500", "wind_z_h850", "total_precipitation_6hr"]
COLS = [FEATURES.index(n) for n in NAMES]
WIND = [c for c, n in enumerate(NAMES) if n.startswith("wind_")]
PLANS = {
    "w1": dict(start="2019-12-01", end="2020-12-30", window_days=1),
    "w61": dict(days=[1, 60, 200, 366], window_days=61),
    "w5g": dict(days=[1, 59, 60, 61, 365, 366], window_days=5, weights="gaussian", sigma_days=1.5),
}


def test_shapes_sit_on_the_kernel_edges():
    from paradis_model_amd import _lib
    assert _lib.lib.paradis_clim_mean_chunk() == CHUNK
    assert [h * w for h, w in GRIDS] == [60, 35, 2 * CHUNK + 64]


@functools.lru_cache(maxsize=None)
def _times():
    t = CO.case_times()
    t.setflags(write=False)
    return t


def _grid(H, W):
    return FO.grid_deg(H, W, False)


@functools.lru_cache(maxsize=None)
def _raw(grid, clean=False):
    H, W = grid
    T = _times().size
    g = torch.Generator().manual_seed(700 + GRIDS.index(grid))
    x = torch.randn(T, len(FEATURES), H, W, generator=g)
    for j, f in enumerate(FEATURES):
        b = FO.base_name(f)
        if b == "temperature":
            x[:, j] = 250.0 + 15.0 * x[:, j]
        elif b == "total_precipitation_6hr":
            x[:, j] = x[:, j].abs() * 1e-3
        else:
            x[:, j] *= 10.0
    if not clean:
        x[::3, :, 0, 1] = float("nan")
        x[:, :, H - 1, W - 2] = float("nan")
        x[::5, :, 1, 0] = float("inf")
    return x


@functools.lru_cache(maxsize=None)
def _store(grid, packing, clean=False):
    from paradis_model_amd.dataset import DeviceStore
    H, W = grid
    lat, lon = _grid(H, W)
    F = len(FEATURES)
    stats = {k: np.ones(F, np.float32) for k in ("mean", "std", "min", "max")}
    return DeviceStore(_raw(grid, clean).numpy(), _times(), FEATURES, stats, lat, lon, np.zeros((H, W, 1), np.float32),
                       toa_mean=0.0, toa_std=1.0, device="cuda", packing=packing)


@functools.lru_cache(maxsize=None)
def _decoded(grid, packing, clean=False):
    """what the store holds, as float32 numpy: the oracle's input, read once and never written"""
    store = _store(grid, packing, clean)
    x = store.rows(0, store.shape[0]).cpu().numpy()
    x.setflags(write=False)
    return x


def _plan(store, key):
    from paradis_model_amd.climatology import ClimPlan
    return ClimPlan(store.times_us, **PLANS[key])


def _oracle_lists(key):
    kw = dict(PLANS[key])
    if "start" in kw:
        kw["start"] = np.datetime64(kw["start"] + "T00:00:00")
        kw["end"] = np.datetime64(kw["end"] + "T23:59:59")
    return CO.slot_lists(_times(), **kw)[0]


@functools.lru_cache(maxsize=None)
def _oracle(grid, packing, key):
    """(fp64 means, float32 climatology without winds, float32 climatology with winds): computed once, shared"""
    lat, lon = _grid(*grid)
    x = _decoded(grid, packing)
    lists = _oracle_lists(key)
    mean, plain, turned = CO.climatology(x, lists, COLS, NAMES, LEVELS, lat, lon)
    for a in (mean, plain, turned):
        a.setflags(write=False)
    return mean, plain, turned


def _spec(**kw):
    from paradis_model_amd.forecast import PostSpec
    C = len(NAMES)
    return PostSpec.from_features(NAMES, LEVELS, zscore_mean=np.zeros(C, np.float32), zscore_std=np.ones(C, np.float32),
                                  custom_normalization=False, dewpoint=False, **kw)


def _same(a, b):
    """bit for bit, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _checksum(store):
    if store.packing is None:
        return (int(store.data.view(torch.int32).long().sum()),)
    return (int(store.codes.view(torch.int16).long().sum()), int(store.plane_params.view(torch.int32).long().sum()))


@pytest.mark.parametrize("key", list(PLANS))
@pytest.mark.parametrize("packing", [None, "u16"])
@pytest.mark.parametrize("grid", GRIDS)
def test_means_within_one_ulp_of_fp64(grid, packing, key):
    from paradis_model_amd import climatology
    store = _store(grid, packing)
    plan = _plan(store, key)
    before = _checksum(store)
    clim = climatology.build(store, plan, names=NAMES, winds=False)
    again = climatology.build(store, plan, _spec(), winds=False)
    torch.cuda.synchronize()
    assert _checksum(store) == before                                   # neither the store nor its codes are written
    H, W = grid
    assert clim.data.shape == (plan.n_slots, len(NAMES), H, W) and clim.data.dtype == torch.float32
    assert clim.data.device == store.device and clim.names == NAMES and clim.plan is plan and not clim.winds
    assert _same(clim.data, again.data)                                 # run == run, names == spec
    got = clim.data.cpu().numpy()
    mean, want, _ = _oracle(grid, packing, key)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert bool(nan[:, :, H - 1, W - 2].all())                          # the all-missing pixel, in every slot
    some = nan[plan.entries > 0][:, :, 0, 1]                            # the pixel that loses every third row
    assert bool(some.any()) and not bool(some.all()) if key == "w1" else not bool(some.any())
    if key == "w1":
        k = plan.days.index(366) * len(plan.hours)
        assert plan.entries[k] == 0 and bool(nan[k].all())              # the slot start / end emptied
        assert int((plan.entries == 0).sum()) == len(plan.hours)
    else:
        assert plan.entries.max() > 8 and bool((plan.entries % 8 != 0).any())
    ok = ~nan
    assert bool(np.isfinite(got[ok]).all())
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    ulp = np.spacing(np.abs(want[ok])).astype(np.float64)
    worst = float((err / ulp).max())
    print(f"CLIM | {grid} | {packing} | {key} | worst error {worst:.2f} ulp | "
          f"max_rel vs fp64 {float(np.abs(got[ok] - mean[ok]).max() / np.abs(mean[ok]).max()):.2e}")
    assert worst <= 1.0


@pytest.mark.parametrize("key", ["w1", "w61"])
@pytest.mark.parametrize("packing", [None, "u16"])
@pytest.mark.parametrize("grid", GRIDS)
def test_winds_of_the_means(grid, packing, key):
    from paradis_model_amd import climatology
    store = _store(grid, packing)
    plan = _plan(store, key)
    spec = _spec()
    plain = climatology.build(store, plan, spec, winds=False).data
    clim = climatology.build(store, plan, spec)
    assert clim.winds and clim.names == NAMES
    got = clim.data
    rest = [c for c in range(len(NAMES)) if c not in WIND]
    assert _same(got[:, rest], plain[:, rest])                          # non-wind channels: untouched
    assert _same(climatology.build(store, plan, spec).data, got)        # run == run
    got = got.cpu().numpy()
    _, _, want = _oracle(grid, packing, key)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    for c in WIND:
        g, r = got[:, c][ok[:, c]].astype(np.float64), want[:, c][ok[:, c]].astype(np.float64)
        e = float(np.abs(g - r).max() / np.abs(r).max())
        print(f"CLIM winds | {grid} | {packing} | {key} | {NAMES[c]} max_rel {e:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert e <= 1e-6, (NAMES[c], e)
        assert float(np.abs(r).max()) > 1.0                             # of the size of its inputs: the bound means something


@pytest.mark.parametrize("grid", [(6, 10), (5, 7)])
def test_spherical_winds_inplace_is_postprocess_bit_for_bit(grid):
    """one expression (csrc/winds.h): identity normalisation through forecast.postprocess == the in-place launch"""
    from paradis_model_amd.climatology import spherical_winds_inplace
    from paradis_model_amd.forecast import postprocess
    H, W = grid
    lat, lon = _grid(H, W)
    spec = _spec()
    K, C = 5, len(NAMES)
    g = torch.Generator().manual_seed(811)
    x = torch.randn(K, C, H, W, generator=g) * 10.0
    x[:, spec.it] = 250.0 + 1.5 * x[:, spec.it]
    xd = x.cuda()
    chunk = torch.zeros(K, 1, C, H, W, device="cuda")
    postprocess(xd, spec, lat, lon, chunk, 0)
    y = xd.clone()
    assert spherical_winds_inplace(y, spec, lat, lon) is y
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)
    assert _same(y, chunk[:, 0])
    assert not torch.equal(y[:, WIND], xd[:, WIND])
    # a NaN in any component gives NaN in all three, and nowhere else
    z = xd.clone()
    z[2, spec.iz[1], 1, 3] = float("nan")
    spherical_winds_inplace(z, spec, lat, lon)
    nan = torch.isnan(z).cpu()
    want = torch.zeros_like(nan)
    want[2, [spec.ix[1], spec.iy[1], spec.iz[1]], 1, 3] = True
    assert torch.equal(nan, want)


def test_out_of_range_entries_are_clamped_and_flagged():
    """the clamp, not a fault: a clamped row or column is valid memory of the store"""
    from paradis_model_amd.climatology import clim_mean
    grid = (6, 10)
    store = _store(grid, None)
    x = _decoded(grid, None)
    T, F = store.shape[:2]
    dev = store.device

    def run(ptr, rows, w, cols):
        out, flag = clim_mean(store, torch.tensor(ptr, dtype=torch.int64, device=dev),
                              torch.tensor(rows, dtype=torch.int64, device=dev),
                              torch.tensor(w, dtype=torch.float64, device=dev),
                              torch.tensor(cols, dtype=torch.int32, device=dev))
        return out.cpu().numpy(), int(flag.item())

    def want(lists, cols):
        return CO.slot_means(x, lists, cols).astype(np.float32)

    got, flag = run([0, 2, 3], [4, 7, 5], [1.0, 3.0, 1.0], [0, 2])
    assert flag == 0
    assert np.array_equal(got, want([[(4, 1.0), (7, 3.0)], [(5, 1.0)]], [0, 2]), equal_nan=True)
    got, flag = run([0, 2, 3], [4, T + 5, -3], [1.0, 3.0, 1.0], [0, 2])                  # rows beyond both ends
    assert flag == 1
    assert np.array_equal(got, want([[(4, 1.0), (T - 1, 3.0)], [(0, 1.0)]], [0, 2]), equal_nan=True)
    got, flag = run([0, 2, 3], [4, 7, 5], [1.0, 3.0, 1.0], [F + 2, -1])                  # columns beyond both ends
    assert flag == 1
    assert np.array_equal(got, want([[(4, 1.0), (7, 3.0)], [(5, 1.0)]], [F - 1, 0]), equal_nan=True)
    got, flag = run([0, 2, 9], [4, 7, 5], [1.0, 3.0, 1.0], [0])                          # a list bound beyond N
    assert flag == 1
    assert np.array_equal(got, want([[(4, 1.0), (7, 3.0)], [(5, 1.0)]], [0]), equal_nan=True)


def test_scorecard_and_forecaster_take_the_climatology_as_it_is():
    from paradis_model_amd import climatology
    from paradis_model_amd.forecast import Forecaster
    from paradis_model_amd.verify import Scorecard
    grid = (6, 10)
    H, W = grid
    store = _store(grid, "u16", True)
    plan = _plan(store, "w1")
    spec = _spec()
    clim = climatology.build(store, plan, spec)
    assert bool(torch.isfinite(clim.data[plan.entries > 0]).all())
    lat, _ = _grid(H, W)
    card = Scorecard(spec.names, np.cos(np.deg2rad(lat)), 2, climatology=clim.data)
    times = store.times_us[[10, 11, 300]]
    idx = clim.index(times)
    assert idx.dtype == torch.int32 and idx.device == store.device and tuple(idx.shape) == (3,)
    assert np.array_equal(idx.cpu().numpy(), plan.slot_of(times))
    g = torch.Generator().manual_seed(5)
    scale = clim.data[idx.long()].abs().mean(dim=(0, 2, 3)).view(1, -1, 1, 1)
    truth = clim.data[idx.long()] + scale * torch.randn(3, len(NAMES), H, W, generator=g).cuda()
    fc = truth + 0.5 * scale * torch.randn(3, len(NAMES), H, W, generator=g).cuda()
    card.update(0, fc, truth, idx)
    empty = clim.index(np.array(["2020-12-31T00"] * 3, "datetime64[us]"))          # the slot start / end emptied
    assert bool(torch.isnan(clim.data[empty.long()]).all())
    card.update(1, fc, truth, empty)
    res = card.result()
    assert bool(np.isfinite(res["acc"][0]).all()) and bool(np.isfinite(res["activity"][0]).all())
    assert bool((res["acc"][0] > 0.5).all()) and bool((res["acc"][0] < 1.0).all())
    assert not bool(np.isfinite(res["acc"][1]).any())
    # Forecaster.run's refusals accept the [B, n_stored] index as it is
    B, n_stored = 2, 3
    valid = store.times_us[torch.tensor([[20, 21, 22], [400, 401, 402]])]
    ci = clim.index(valid)
    assert ci.dtype == torch.int32 and tuple(ci.shape) == (B, n_stored)
    card3 = Scorecard(spec.names, np.cos(np.deg2rad(lat)), n_stored, climatology=clim.data)
    me = types.SimpleNamespace(spec=spec, _truth={})
    tr = torch.zeros(B, n_stored, len(NAMES), H, W, device="cuda")
    assert Forecaster._check_verification(me, card3, tr, False, ci, B, n_stored, len(NAMES), H, W) is None
    with pytest.raises(ValueError, match="clim_index"):
        Forecaster._check_verification(me, card3, tr, False, ci.long(), B, n_stored, len(NAMES), H, W)
