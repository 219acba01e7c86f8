"""Host side of the device-resident dataset (paradis_model_amd/dataset.py), no GPU: the batch oracle decodes an
identity-coded store to the (time, feature) pairs that data/era5_dataset.py:338-354 prescribes; DeviceDataset's feature
orders, counts, normalisation tables, length and base; DeviceLoader's index streams; the argument checks of
paradis_assemble_batch, which return before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from paradis_model_amd.config import feature_layout
from tests import batch_oracle as BO


# ---------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("n_t", [1, 2, 3])
@pytest.mark.parametrize("interval,shift", [(1, 0), (2, 0), (1, 1), (2, 1)])
@pytest.mark.parametrize("S", [1, 3])
def test_oracle_decodes_identity_store(n_t, interval, shift, S):
    """store[t, f, y, x] = t*F + f + (y*W + x)/4096, z-score with mean 0 / std 1: plane value at cell 0 is t*F + f.  The
    expected (t, f) are written out from era5_dataset.py:338-354, not taken from the oracle's own slicing."""
    H, W = 3, 5
    # a store long enough for every override below (delta_steps only sizes the store here)
    case = BO.build_case(H, W, n_time_inputs=n_t, interval_steps=2, delta_steps=2, steps=3, n_samples=3, base=2,
                         identity=True)
    F = len(case.features)
    cell = (torch.arange(H * W, dtype=torch.float32) / 4096).view(H, W)
    for ind in (0, 2):
        x, y, forc = BO.item(case, ind, n_time_inputs=n_t, interval_steps=interval, prediction_shift=shift, steps=S)
        Fin, Fout = len(case.in_cols), len(case.out_cols)
        assert x.shape == (1, n_t * Fin, H, W) and y.shape == (S, Fout, H, W)
        assert forc.shape == (S, H, W, 5 * n_t)
        t_in = case.base + ind * interval                     # input_ini, in rows of the store
        for k in range(n_t):
            for j in range(Fin):
                want = float((t_in + k) * F + case.in_cols[j])
                assert torch.equal(x[0, k * Fin + j], want + cell), (k, j)
        t_out = t_in + n_t + shift                            # output_ini
        for s in range(S):
            for j in range(Fout):
                want = float((t_out + s) * F + case.out_cols[j])
                assert torch.equal(y[s, j], want + cell), (s, j)
        xp, yp, fp = BO.item(case, ind, n_time_inputs=n_t, interval_steps=interval, prediction_shift=shift, steps=S,
                             prediction=True)
        assert yp is None and torch.equal(xp, x) and torch.equal(fp, forc)


def test_builder_has_every_feature_class():
    case = BO.build_case(3, 5)
    n_c = case.n_common
    assert 0 < n_c < len(case.in_names) and n_c < len(case.out_names)          # input-only and output-only exist
    assert case.in_names[:n_c] == case.out_names[:n_c]
    assert case.in_names[n_c:] == ["wind_z_10m"]
    assert "total_precipitation_6hr" in case.out_names[n_c:]
    assert any(n.startswith("specific_humidity_h") for n in case.in_names)
    assert len(case.features) == len(set(case.in_names + case.out_names)) + 2  # two features nothing uses
    assert case.features != sorted(case.features)                              # shuffled store order
    assert BO.FO.KIND_HUMIDITY in case.norm_in[0] and BO.FO.KIND_PRECIP in case.norm_out[0]


# ---------------------------------------------------------------------------------- DeviceDataset bookkeeping
@pytest.mark.parametrize("n_t,interval,delta,S", [(2, 1, 1, 1), (3, 2, 2, 3), (1, 1, 2, 1)])
def test_dataset_bookkeeping(n_t, interval, delta, S):
    from paradis_model_amd import feed
    case = BO.build_case(3, 5, n_time_inputs=n_t, interval_steps=interval, delta_steps=delta, steps=S, n_samples=5,
                         base=2)
    ds = BO.make_dataset(case, "cpu")
    lay = feature_layout(case.cfg)
    assert ds.dyn_input_features == case.in_names and ds.dyn_output_features == case.out_names
    assert ds.num_common_features == lay.num_common_features == case.n_common
    assert ds.num_out_features == lay.num_out_features == len(case.out_names)
    assert ds.num_dyn_inputs_single == lay.dyn_single
    assert ds.num_in_dyn_features == lay.num_in_dyn_features
    assert ds.num_in_static_features == lay.num_in_static_features
    assert ds.num_in_features == lay.num_in_dyn_features + lay.num_in_static_features
    assert ds.output_name_order == lay.output_name_order
    assert ds.dataset is ds and ds.lat_size == 3 and ds.lon_size == 5
    assert torch.equal(ds.lat, case.lat) and torch.equal(ds.lon, case.lon)
    assert (ds.n_time_inputs, ds.interval_steps, ds.prediction_shift) == (n_t, interval, (delta - 1) * interval)
    assert len(ds) == 5 and ds.base == 2
    assert ds.time[0] == np.datetime64(case.start_date) and ds.time[-1] == np.datetime64(case.end_date)
    # normalisation tables against the oracle's independent restatement
    for got, want in (((ds.kind_in, ds.p0_in, ds.p1_in), case.norm_in), ((ds.kind_out, ds.p0_out, ds.p1_out), case.norm_out)):
        assert got[0].tolist() == want[0]
        assert np.array_equal(got[1], want[1].numpy()) and np.array_equal(got[2], want[2].numpy())
    assert feed.KIND_HUMIDITY in ds.kind_in and feed.KIND_PRECIP in ds.kind_out and feed.KIND_PRECIP not in ds.kind_in
    assert float(ds.q_max) == float(case.q_max) and float(ds.q_min) == float(case.q_min) > 1e-12
    # the plane table: input channel k*Fin + j at time offset k; target step s at n_t + shift + s
    Fin, Fout = len(case.in_names), len(case.out_names)
    tab = ds.plane_table
    assert tab.shape == (n_t * Fin + S * Fout,) and tab.dtype.itemsize == 20
    for k in range(n_t):
        rows = tab[k * Fin:(k + 1) * Fin]
        assert rows["feature"].tolist() == case.in_cols and set(rows["dt"].tolist()) == {k}
        assert rows["kind"].tolist() == case.norm_in[0]
    for s in range(S):
        rows = tab[n_t * Fin + s * Fout:n_t * Fin + (s + 1) * Fout]
        assert rows["feature"].tolist() == case.out_cols
        assert set(rows["dt"].tolist()) == {n_t + (delta - 1) * interval + s}
        assert np.array_equal(rows["p0"], case.norm_out[1].numpy()) and np.array_equal(rows["p1"], case.norm_out[2].numpy())


def test_dataset_standard_normalisation_and_q_min_floor():
    from paradis_model_amd import feed
    case = BO.build_case(3, 5, q_min_floor=True)
    ds = BO.make_dataset(case, "cpu")
    assert float(ds.q_min) == float(np.float32(1e-12)) == float(case.q_min)       # raised from 0 (era5_dataset.py:536-537)
    hum = ds.kind_in == feed.KIND_HUMIDITY
    assert hum.any() and np.all(ds.p0_in[hum] == np.float32(1e-12)) and np.all(ds.p1_in[hum] == ds.q_max)
    assert np.all(ds.p0_out[ds.kind_out == feed.KIND_HUMIDITY] == np.float32(1e-12))   # the output side: the same pair
    case.cfg.normalization.standard = True
    ds = BO.make_dataset(case, "cpu")
    assert set(ds.kind_in.tolist()) == {feed.KIND_ZSCORE} == set(ds.kind_out.tolist())
    col = {n: j for j, n in enumerate(case.features)}
    assert np.array_equal(ds.p0_out, case.stats["mean"][[col[n] for n in case.out_names]])
    assert np.array_equal(ds.p1_in, case.stats["std"][[col[n] for n in case.in_names]])


def test_dataset_length_follows_the_date_range():
    from paradis_model_amd.dataset import DeviceDataset
    case = BO.build_case(3, 5, n_time_inputs=2, interval_steps=2, delta_steps=1, steps=1, n_samples=6, base=1)
    store = BO.make_store(case, "cpu")
    t = case.times
    # start at store row 2 (base 1); an end between two sampled times keeps the earlier one
    for end_row, want in ((2, 1), (3, 1), (4, 2), (7, 3), (12, 6)):
        ds = DeviceDataset(store, case.cfg, case.start_date, str(t[end_row].astype("datetime64[s]")), 1)
        assert len(ds) == want == len(range(2, end_row + 1, 2)) and ds.base == 1
    # a date without a clock: 00:00:00 for the start, 23:59:59 for the end (era5_dataset.py:98-99,124-125)
    ds = DeviceDataset(store, case.cfg, "2000-02-28", "2000-02-28", 1)
    lo = int(np.searchsorted(t, np.datetime64("2000-02-28T00:00:00")))
    assert ds.base == lo - 1 and len(ds) == 2                                     # 00h and 12h of that day
    assert len(DeviceDataset(store, case.cfg, case.start_date, str(t[1].astype("datetime64[s]")), 1)) == 0


def test_dataset_value_errors():
    from paradis_model_amd.dataset import DeviceDataset, DeviceStore
    case = BO.build_case(3, 5, n_time_inputs=2, steps=2, n_samples=4, base=1)
    store = BO.make_store(case, "cpu")
    late = str((case.times[-1]).astype("datetime64[s]"))
    with pytest.raises(ValueError, match="of the last sample"):
        DeviceDataset(store, case.cfg, case.start_date, late, case.steps)
    with pytest.raises(ValueError, match="inputs of the last sample"):
        DeviceDataset(store, case.cfg, case.start_date, late, case.steps, prediction_stage=True)
    # the prediction stage needs no targets: the range that is too long above fits once the targets are not read
    almost = str((case.times[-2]).astype("datetime64[s]"))
    with pytest.raises(ValueError, match="targets"):
        DeviceDataset(store, case.cfg, case.start_date, almost, case.steps)
    assert len(DeviceDataset(store, case.cfg, case.start_date, almost, case.steps, prediction_stage=True)) > 4
    with pytest.raises(ValueError, match="first sample"):
        DeviceDataset(store, case.cfg, str(case.times[0].astype("datetime64[s]")), case.end_date, case.steps)
    names = list(case.features)
    gone = case.in_names[3]
    names[names.index(gone)] = "renamed"
    short = DeviceStore(case.store.numpy(), case.times, names, case.stats, case.lat, case.lon, case.constants, 0.0, 1.0,
                        device="cpu")
    with pytest.raises(ValueError, match=gone):
        DeviceDataset(short, case.cfg, case.start_date, case.end_date, case.steps)
    with pytest.raises(ValueError, match="ascending"):
        DeviceStore(case.store.numpy(), case.times, case.features, case.stats, case.lat.flip(0), case.lon,
                    case.constants, 0.0, 1.0, device="cpu")
    with pytest.raises(ValueError, match="float32"):
        DeviceStore(case.store.double().numpy(), case.times, case.features, case.stats, case.lat, case.lon,
                    case.constants, 0.0, 1.0, device="cpu")
    # host indices are range-checked before anything else; a CPU store has no batch path at all
    ds = BO.make_dataset(case, "cpu")
    with pytest.raises(IndexError):
        ds.batch([0, len(ds)])
    with pytest.raises(IndexError):
        ds.batch(torch.tensor([-1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ds.batch([0])


# ---------------------------------------------------------------------------------- DeviceLoader index streams
def test_epoch_indices():
    from paradis_model_amd.dataset import batch_bounds, epoch_indices
    n = 23
    assert epoch_indices(n).tolist() == list(range(n))
    a, b = epoch_indices(n, 3, True, seed=7), epoch_indices(n, 3, True, seed=7)
    assert torch.equal(a, b) and sorted(a.tolist()) == list(range(n)) and a.tolist() != list(range(n))
    assert not torch.equal(a, epoch_indices(n, 4, True, seed=7))
    assert torch.equal(epoch_indices(n, 4, True, seed=7), epoch_indices(n, 3, True, seed=8))      # seed + epoch
    assert torch.equal(a, torch.randperm(n, generator=torch.Generator().manual_seed(10)))
    # ranks partition the permutation padded by wrapping (DistributedSampler's rule)
    world = 4
    parts = [epoch_indices(n, 3, True, seed=7, rank=r, world_size=world) for r in range(world)]
    assert all(p.numel() == 6 for p in parts)
    padded = torch.cat([a, a[:1]])
    assert torch.equal(torch.stack(parts, 1).reshape(-1), padded)
    assert epoch_indices(2, 0, False, rank=2, world_size=5).tolist() == [0]                       # wraps more than once
    with pytest.raises(ValueError):
        epoch_indices(n, rank=4, world_size=4)
    assert batch_bounds(23, 5, False) == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 23)]
    assert batch_bounds(23, 5, True) == [(0, 5), (5, 10), (10, 15), (15, 20)]
    assert batch_bounds(4, 5, True) == [] and batch_bounds(0, 5, False) == []


def test_loader_lengths_without_a_device():
    from paradis_model_amd.dataset import DeviceLoader
    case = BO.build_case(3, 5, n_samples=7)
    ds = BO.make_dataset(case, "cpu")
    assert len(DeviceLoader(ds, 3)) == 3 and len(DeviceLoader(ds, 3, drop_last=True)) == 2
    ld = DeviceLoader(ds, 2, shuffle=True, seed=5, rank=1, world_size=2)
    assert len(ld) == 2 and ld.indices().numel() == 4
    first = ld.indices()
    ld.set_epoch(1)
    assert not torch.equal(first, ld.indices())


# ---------------------------------------------------------------------------------- the C entry point's checks
def test_assemble_batch_argument_validation_without_gpu():
    """Rejected arguments return 1 with a message before any HIP call; B == 0 returns 0 and launches nothing."""
    from paradis_model_amd import _lib
    L = _lib.lib
    tab = ctypes.cast(ctypes.create_string_buffer(20 * 8), ctypes.c_void_p)     # a non-null table; never read on the host

    def call(T=4, F=3, H=2, W=2, B=1, interval=1, table=tab, n_t=1, Fin=1, S=1, Fout=1):
        return L.paradis_assemble_batch(None, T, F, H, W, None, B, 0, interval, table, n_t, Fin, S, Fout, None, None,
                                        1e-12, None, None)
    assert call(n_t=0) == 1 and "n_time_inputs" in _lib.last_error()
    assert call(S=-1) == 1 and "S=-1" in _lib.last_error()
    assert call(T=0) == 1 and "shape" in _lib.last_error()
    assert call(H=0) == 1 and call(W=-2) == 1 and call(F=0) == 1 and call(B=-1) == 1
    assert call(Fin=0) == 1 and call(Fout=-1) == 1
    assert call(interval=0) == 1 and "interval" in _lib.last_error()
    assert call(table=None) == 1 and "table" in _lib.last_error()
    assert call(B=0, table=None) == 1                                           # a null table is refused whatever B
    assert call() == 1 and "pointers" in _lib.last_error()                      # null store / idx / input / flag
    assert call(B=0) == 0 and call(B=0, S=0, Fout=0) == 0
    assert L.paradis_assemble_batch_chunk() == 2048
    assert L.paradis_abi_version() == 10
