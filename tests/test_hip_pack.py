"""GPU: the 16-bit packed device store (paradis_model_amd/dataset.py ``DeviceStore(packing="u16")``, csrc/feed.hip
``paradis_pack_planes`` / ``paradis_unpack_planes`` / ``paradis_assemble_batch_packed``) against the numpy restatement
of tests/pack_oracle.py, and the contract: a batch from a packed store equals, bit for bit, the float32 batch
assembled from the store's decoded rows.

Shapes sit on the kernels' edges.  The assembly and unpack launches work in chunks of
``paradis_assemble_batch_chunk()`` = 2048 values of a plane, four codes per 8-byte load where P % 4 == 0:
  (3, 5)    P = 15: odd, scalar path, smaller than a wave
  (4, 6)    P = 24: vector path
  (32, 64)  P = 2048: exactly one chunk
  (36, 57)  P = 2052: one chunk + 4, P % 8 != 0
  (3, 683)  P = 2049: odd, one chunk + 1
  (64, 64)  P = 4096: two chunks
The pack launch splits a plane into pieces of ``paradis_pack_planes_piece()`` = 8192 values whose minima and maxima are
folded again by the quantising pass; pack and unpack also run at
  (72, 114) P = 8208: a second piece of 16 values, vector path
  (3, 2731) P = 8193: a second piece of one value, scalar path
T = 6 for the pack / unpack / statistics tests; the contract runs the (n_t, S, interval, delta) of
test_hip_dataset.CONFIGS, whose stores are as long as their last sample needs.  Every comparison is exact (bits, NaN
equal to NaN) except the decode error, which is held to the bounds of tests/pack_oracle.py.
"""
import functools
import re

import numpy as np
import pytest
import torch

from tests import batch_oracle as BO
from tests import pack_oracle as PK
from tests.test_hip_dataset import CONFIGS, INDICES, _e2e_case, _train_setup

pytestmark = pytest.mark.gpu

CHUNK, PIECE = 2048, 8192
SHAPES = [(3, 5), (4, 6), (32, 64), (36, 57), (3, 683), (64, 64)]
PACK_SHAPES = SHAPES + [(72, 114), (3, 2731)]
FULL = ((4, 6), True)                      # the one case with the unmodified feature list


def test_shapes_sit_on_the_kernel_edges():
    from paradis_model_amd import _lib
    assert _lib.lib.paradis_assemble_batch_chunk() == CHUNK and _lib.lib.paradis_pack_planes_piece() == PIECE
    sizes = [h * w for h, w in SHAPES]
    assert sizes == [15, 24, CHUNK, CHUNK + 4, CHUNK + 1, 2 * CHUNK]
    assert [h * w for h, w in PACK_SHAPES[len(SHAPES):]] == [PIECE + 16, PIECE + 1]


def _domains(features):
    return [PK.LOG if re.sub(r"_h\d+$", "", f) == "total_precipitation_6hr" else PK.LINEAR for f in features]


def _plant(case):
    """NaN, both infinities, a constant plane and an all-missing plane, in linear planes and in the log-domain one"""
    x = case.store                                   # this module's own case: written once, here
    T, F, H, W = x.shape
    precip = _domains(case.features).index(PK.LOG)
    lin = [f for f in case.in_cols if f != precip]   # input features: whatever the sample, they are in its batch
    x[:, lin[0], 0, 0] = float("nan")
    x[2, lin[1], H - 1, W - 1] = float("inf")
    x[0, lin[2], 0, 1] = float("-inf")
    x[3, lin[3]] = 5.0
    x[4, lin[4]] = float("nan")
    x[T - 1, lin[5], H // 2] = float("inf")
    x[2, precip, 0, 0] = float("nan")
    x[3, precip, H - 1, W - 1] = float("inf")
    x[5 % T, precip] = 0.0                           # constant in the log domain
    return case


@functools.lru_cache(maxsize=None)
def _case(shape, config=CONFIGS[0], full=False):
    B, n_t, S, interval, delta = config
    case = BO.build_case(*shape, n_time_inputs=n_t, interval_steps=interval, delta_steps=delta, steps=S, n_samples=4,
                         base=1, full=full, seed=40 + PACK_SHAPES.index(shape) + 10 * CONFIGS.index(config))
    return _plant(case)


@functools.lru_cache(maxsize=None)
def _oracle(shape, full=False):
    """(codes, params, decoded) of the T = 6 case by the numpy restatement: computed once, shared, never written"""
    case = _case(shape, CONFIGS[0], full)
    assert case.store.shape[0] == 6
    dom = _domains(case.features)
    codes, params = PK.pack_store(case.store.numpy(), dom)
    back = PK.unpack_store(codes, params, dom)
    for a in (codes, params, back):
        a.setflags(write=False)
    return codes, params, back


def _store(case, packing="u16", stats=True, data=None):
    from paradis_model_amd.dataset import DeviceStore
    return DeviceStore(case.store.numpy() if data is None else data, case.times, case.features,
                       case.stats if stats else None, case.lat, case.lon, case.constants, case.toa_mean, case.toa_std,
                       device="cuda", packing=packing)


def _float_store_of(case, packed):
    return _store(case, packing=None, data=packed.rows(0, packed.shape[0]))


def _dataset(case, store, **kw):
    from paradis_model_amd.dataset import DeviceDataset
    return DeviceDataset(store, case.cfg, case.start_date, case.end_date, case.steps, **kw)


def _same(a, b):
    """bit for bit, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _codes_np(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


CASES = [(s, False) for s in PACK_SHAPES] + [FULL]


# ---------------------------------------------------------------------------------- 1. pack against the oracle
@pytest.mark.parametrize("shape,full", CASES)
def test_pack_equals_the_oracle(shape, full):
    from paradis_model_amd.dataset import pack_planes
    case = _case(shape, CONFIGS[0], full)
    codes, params, _ = _oracle(shape, full)
    dom = _domains(case.features)
    assert {PK.LINEAR, PK.LOG} == set(dom)
    store = _store(case)
    assert store.packing == "u16" and store.data is None and store.domain.tolist() == dom
    assert store.codes.dtype == torch.uint16 and store.codes.shape == case.store.shape
    assert store.plane_params.shape == case.store.shape[:2] + (2,)
    assert store.nbytes == case.store.numel() * 2 + case.store.shape[0] * case.store.shape[1] * 8
    got_c, got_p = _codes_np(store.codes), store.plane_params.cpu().numpy()
    bad = np.argwhere((got_p.view(np.int32) != params.view(np.int32)).any(-1))
    print(f"{shape}: planes whose (lo, s) differ from the oracle's: {len(bad)}; codes that differ: "
          f"{int((got_c != codes).sum())} of {codes.size}")
    assert np.array_equal(got_p.view(np.int32), params.view(np.int32)), bad[:5]
    assert np.array_equal(got_c, codes)
    # two calls are bit-identical, and a slab packed in two pieces (rows [0, 2) and [2, 6)) equals the slab packed whole
    slab = case.store.cuda()
    for pieces in ([(0, 6)], [(0, 6)], [(2, 6), (0, 2)]):
        c2 = torch.full_like(store.codes.view(torch.int16), 0x1111)
        p2 = torch.full_like(store.plane_params, -7.0)
        for a, b in pieces:
            pack_planes(slab[a:b], a, c2.view(torch.uint16), p2, store.domain_dev)
        assert torch.equal(c2, store.codes.view(torch.int16)), pieces
        assert torch.equal(p2.view(torch.int32), store.plane_params.view(torch.int32)), pieces


# ---------------------------------------------------------------------------------- 2. unpack
@pytest.mark.parametrize("shape,full", CASES)
def test_rows_equal_the_oracle_decode_within_the_bound(shape, full):
    case = _case(shape, CONFIGS[0], full)
    _, params, back = _oracle(shape, full)
    store = _store(case)
    T = store.shape[0]
    got = store.rows(0, T)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == case.store.shape
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.int32), back.view(np.int32)) or np.array_equal(got, back, equal_nan=True)
    assert np.array_equal(store.rows(2, 5).cpu().numpy(), back[2:5], equal_nan=True)
    assert store.rows(3, 3).shape[0] == 0
    with pytest.raises(IndexError):
        store.rows(0, T + 1)
    # against the original: missing exactly where it is not finite, within the bound elsewhere
    x = case.store.numpy()
    for f, d in enumerate(_domains(case.features)):
        for t in range(T):
            o, g = x[t, f], got[t, f]
            if d == PK.LOG:
                with np.errstate(invalid="ignore", divide="ignore"):
                    fin = np.isfinite(np.log(o + np.float32(1e-6)))
            else:
                fin = np.isfinite(o)
            assert np.array_equal(np.isnan(g), ~fin), (t, f)
            if not fin.any():
                continue
            if d == PK.LOG:
                err = np.abs(PK.normalise_precip(g[fin]).astype(np.float64) - PK.normalise_precip(o[fin])).max()
                assert err <= PK.precip_bound(params[t, f, 1]), (t, f, err)
            else:
                err = np.abs(g[fin].astype(np.float64) - o[fin]).max()
                assert err <= PK.linear_bound(o[fin].min(), o[fin].max()), (t, f, err)


# ---------------------------------------------------------------------------------- 3. the contract
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_packed_batch_equals_the_float_batch_of_the_decoded_store(shape, config):
    case = _case(shape, config)
    packed = _store(case)
    plain = _float_store_of(case, packed)
    assert plain.packing is None and plain.data is not None
    idx = INDICES[config[0]]
    dp, df = _dataset(case, packed), _dataset(case, plain)
    got, want = dp.batch(idx), df.batch(idx)
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and g.is_contiguous() and _same(g, w)
    assert torch.isnan(got[0]).any() or torch.isnan(got[1]).any()          # the planted planes are in the batch
    # the prediction-stage item: no target
    gp = _dataset(case, packed, prediction_stage=True).batch(idx)
    wp = _dataset(case, plain, prediction_stage=True).batch(idx)
    assert len(gp) == 4 and gp[0].tolist() == idx
    for g, w in zip(gp[1:], wp[1:]):
        assert _same(g, w)
    assert _same(gp[1], got[0])
    assert dp.index_errors() == 0 and df.index_errors() == 0


def test_contract_with_every_kind_and_the_log_domain():
    from paradis_model_amd.feed import KIND_HUMIDITY, KIND_PRECIP, KIND_ZSCORE
    case = _case(FULL[0], CONFIGS[1], True)
    packed = _store(case)
    plain = _float_store_of(case, packed)
    dp, df = _dataset(case, packed), _dataset(case, plain)
    assert set(dp.kind_in.tolist()) | set(dp.kind_out.tolist()) == {KIND_ZSCORE, KIND_HUMIDITY, KIND_PRECIP}
    assert packed.domain[dp.out_columns].tolist().count(PK.LOG) == 1
    for g, w in zip(dp.batch(INDICES[3]), df.batch(INDICES[3])):
        assert _same(g, w)


# ---------------------------------------------------------------------------------- 4. alignment
@pytest.mark.parametrize("shape", [(4, 6), (36, 57)])
def test_unaligned_pointers_take_the_scalar_path_with_the_same_values(shape):
    from paradis_model_amd import _lib
    from paradis_model_amd.dataset import EPS_Q
    case = _case(shape, CONFIGS[1])
    store = _store(case)
    ds = _dataset(case, store)
    idx = torch.tensor(INDICES[3], device="cuda")
    inp, tgt, _, _ = ds.batch(idx)
    T, F, H, W = store.shape
    assert (H * W) % 4 == 0 and store.codes.data_ptr() % 8 == 0 and inp.data_ptr() % 16 == 0

    def call(codes_ptr, inp_ptr, tgt_ptr):
        rc = _lib.lib.paradis_assemble_batch_packed(codes_ptr, store.plane_params.data_ptr(), store.domain_dev.data_ptr(),
                                                    T, F, H, W, idx.data_ptr(), 3, ds.base, ds.interval_steps,
                                                    ds._planes.data_ptr(), ds.n_time_inputs, ds.num_dyn_inputs_single,
                                                    ds.forecast_steps, ds.num_out_features, inp_ptr, tgt_ptr, EPS_Q,
                                                    ds._flag.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "assemble_batch_packed")

    # input offset by 4 bytes
    buf = torch.zeros(inp.numel() + 4, device="cuda")
    t2 = torch.zeros_like(tgt)
    call(store.codes.data_ptr(), buf.data_ptr() + 4, t2.data_ptr())
    assert _same(buf[1:1 + inp.numel()], inp.reshape(-1)) and _same(t2, tgt)
    assert buf[0] == 0 and not buf[1 + inp.numel():].any()
    # codes offset by 2 bytes
    shifted = torch.zeros(store.codes.numel() + 4, dtype=torch.int16, device="cuda")
    shifted[1:1 + store.codes.numel()] = store.codes.view(torch.int16).reshape(-1)
    i3, t3 = torch.zeros_like(inp), torch.zeros_like(tgt)
    call(shifted.data_ptr() + 2, i3.data_ptr(), t3.data_ptr())
    assert _same(i3, inp) and _same(t3, tgt)
    assert ds.index_errors() == 0


# ---------------------------------------------------------------------------------- 5. clamping
def test_out_of_range_device_indices_are_clamped_and_flagged_like_the_float_path():
    case = _case((4, 6), CONFIGS[1])
    packed = _store(case)
    plain = _float_store_of(case, packed)
    T, F, H, W = packed.shape
    # a canary row before and after both arrays: codes that decode to something else, parameters that blow up
    big_c = torch.full((T + 2, F, H, W), 12345, dtype=torch.int16, device="cuda")
    big_p = torch.full((T + 2, F, 2), 1e30, device="cuda")
    big_c[1:T + 1] = packed.codes.view(torch.int16)
    big_p[1:T + 1] = packed.plane_params
    packed.codes, packed.plane_params = big_c[1:T + 1].view(torch.uint16), big_p[1:T + 1]
    assert packed.codes.is_contiguous() and packed.plane_params.is_contiguous()
    n = case.n_samples
    good = INDICES[3]
    idx = torch.tensor([good[0], n, good[1], -5, good[2], n + 3, 2 ** 62, -2 ** 62], device="cuda")
    dp, df = _dataset(case, packed), _dataset(case, plain)
    assert dp.batch(torch.tensor(good, device="cuda"))[0].shape[0] == 3 and dp.index_errors() == 0
    got, want = dp.batch(idx), df.batch(idx)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert _same(g, w)
    assert dp.index_errors() != 0 and df.index_errors() != 0
    assert dp.index_errors(clear=True) != 0 and dp.index_errors() == 0
    assert torch.equal(big_c[0], torch.full_like(big_c[0], 12345)) and bool((big_p[[0, -1]] == 1e30).all())
    for host in ([good[0], n], [-5]):
        with pytest.raises(IndexError):
            dp.batch(host)
    assert dp.index_errors() == 0


# ---------------------------------------------------------------------------------- 6. empty batch, out=, capture, loader
def test_empty_batch_out_tensors_capture_and_loader():
    from paradis_model_amd.dataset import DeviceLoader, epoch_indices
    from paradis_model_amd.harness import capture_forward
    case = _case((36, 57), CONFIGS[1])
    packed = _store(case)
    plain = _float_store_of(case, packed)
    dp, df = _dataset(case, packed), _dataset(case, plain)
    empty = dp.batch([])
    assert [tuple(t.shape) for t in empty] == [tuple(s) for s in dp.batch_shapes(0)]
    assert dp.batch(torch.empty(0, dtype=torch.int64, device="cuda"))[1].shape == empty[1].shape
    want = [t.clone() for t in df.batch(INDICES[3])]
    out = tuple(torch.full(s, float("inf"), device="cuda") for s in dp.batch_shapes(3))
    got = dp.batch(INDICES[3], out=out)
    assert all(g is o for g, o in zip(got, out))
    for g, w in zip(got, want):
        assert _same(g, w)
    # captured in a HIP graph, replayed with new indices
    idx = torch.tensor([0, 1, 2], device="cuda")
    static = tuple(torch.zeros(s, device="cuda") for s in dp.batch_shapes(3))
    graph, res = capture_forward(lambda: dp.batch(idx, out=static))
    assert all(r is s for r, s in zip(res, static))
    idx.copy_(torch.tensor(INDICES[3], device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(static, want):
        assert _same(g, w)
    # the loader
    loader = DeviceLoader(dp, 3, shuffle=True, seed=4)
    loader.set_epoch(2)
    order = epoch_indices(len(dp), 2, True, 4).tolist()
    batches = [[t.clone() for t in bt] for bt in loader]
    assert len(batches) == 2
    for k, bt in enumerate(batches):
        for g, w in zip(bt, df.batch(order[3 * k:3 * k + 3])):
            assert _same(g, w)
    assert dp.index_errors() == 0


# ---------------------------------------------------------------------------------- 7. statistics
def test_statistics_come_from_the_original_values_slab_by_slab(monkeypatch):
    from paradis_model_amd import dataset
    from paradis_model_amd.prepare import StoreStats
    case = _case((4, 6))
    T, F, H, W = case.store.shape
    assert T == 6
    monkeypatch.setattr(dataset, "SLAB_BYTES", 2 * F * H * W * 4)          # two rows per slab: three slabs
    store = _store(case, stats=False)
    mine = StoreStats(F, H, W, device="cuda")
    for a in range(0, T, 2):
        mine.update(case.store[a:a + 2].cuda())
    want = mine.result()
    assert set(store.stats) == {"mean", "std", "min", "max"}
    for key in store.stats:
        assert store.stats[key].dtype == np.float32
        assert np.array_equal(store.stats[key].view(np.int32), want[key].view(np.int32)), key
    # and the codes do not depend on the slab boundaries
    monkeypatch.undo()
    whole = _store(case)
    assert torch.equal(store.codes.view(torch.int16), whole.codes.view(torch.int16))
    assert torch.equal(store.plane_params.view(torch.int32), whole.plane_params.view(torch.int32))
    # +Inf reaches the statistics of the original values; a decoded store would have lost it
    assert np.isinf(store.stats["max"]).any()


# ---------------------------------------------------------------------------------- 8. initial state
def test_initial_state_on_a_packed_dataset():
    from paradis_model_amd.encode import initial_state
    from paradis_model_amd.feed import KIND_ZSCORE
    from paradis_model_amd.forecast import PostSpec
    case = _e2e_case()
    packed = _store(case)
    plain = _float_store_of(case, packed)
    res = []
    for store in (packed, plain):
        ds = _dataset(case, store, prediction_stage=True)
        nz = int((ds.kind_out == KIND_ZSCORE).sum())
        post = PostSpec.from_features(ds.dyn_output_features, list(case.cfg.features.pressure_levels),
                                      zscore_mean=np.zeros(nz, np.float32), zscore_std=np.ones(nz, np.float32),
                                      q_min=float(ds.q_min), q_max=float(ds.q_max), custom_normalization=True)
        res.append(initial_state(ds, [1, 3], post, case.lat.double().numpy(), case.lon.double().numpy()))
        assert ds.index_errors() == 0
    (s0, d0), (s1, d1) = res
    assert s0.shape[0] == 2 and bool(torch.isfinite(s0).any())
    assert _same(s0, s1) and _same(d0, d1)


# ---------------------------------------------------------------------------------- 9. end to end
def test_train_step_fed_from_a_packed_store():
    case = _e2e_case()
    packed = _store(case)
    plain = _float_store_of(case, packed)
    dp, df = _dataset(case, packed), _dataset(case, plain)
    loss_p = float(_train_setup(case, dp, False)(dp.batch([1, 3])))
    loss_f = float(_train_setup(case, df, False)(df.batch([1, 3])))
    assert np.isfinite(loss_p) and loss_p == loss_f
