"""GPU: the forecast writer's layout on the device (paradis_model_amd/encode.py, csrc/encode.hip::paradis_forecast_encode)
against the numpy restatement of tests/encode_oracle.py, ``initial_state`` against the reference's own wind conversion
and dew point (golden e1_encode.pt), and ``Forecaster.run(encoder=...)`` against the oracle applied to the chunks the
same forecaster delivers without an encoder.

The encoding is a bit operation: every comparison of encoded values is EXACT, on int32 views.  Shapes: B = 2, C = 97,
L = 13; 8x16 (P = 128: the 16-byte path, one segment per plane, half of its lanes) and 5x6 (P = 30, not a multiple of
four: the scalar path); n in {1, 3}; the first chunk (``td_off = 1``) and a later one.  ``P`` beyond one segment
(EN_CHUNK = 2048 values) is the 33x64 case.  Bounds of ``initial_state``: those of tests/test_hip_forecast.py - winds
are float64 expressions of the stored fp32 values rounded once, 1e-6 against the reference on a float64 grid; the dew
point 1e-6 against the formula on the kernel's own q and T; gathered channels are the store's bits."""
import functools

import numpy as np
import pytest
import torch

from paradis_model_amd.config import default_config, feature_layout, reduced_config, stub_datamodule
from tests import encode_oracle as EO
from tests import forecast_oracle as FO
from tests._util import load_golden, max_rel, seeded

pytestmark = pytest.mark.gpu

B, C, L = 2, 97, 13
SENTINEL = 0x5A5A5A5A
# NaN with every mantissa bit, the quiet NaN, +-inf, +-0, denormals, the largest finite number, and mantissas that end
# in exactly half a quantum above an even and above an odd kept bit: 0x40 at keepbits 16, 0x200000 at keepbits 1
PATTERNS = [0x7FFFFFFF, 0x7FC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000001,
            0x7F7FFFFF, 0xFF7FFFFF, 0x3F800040, 0x3F8000C0, 0xBF800040, 0xBF8000C0, 0x3F200000, 0x3F600000]
KEEPBITS = [16, 1, 23, None]


@functools.lru_cache(maxsize=None)
def _setup():
    from paradis_model_amd.encode import EncodeSpec
    cfg = default_config()
    names = feature_layout(cfg).output_name_order
    levels = list(cfg.features.pressure_levels)
    specs = {k: EncodeSpec.from_config(cfg, names, levels, keepbits=k) for k in KEEPBITS}
    return cfg, names, levels, specs


@functools.lru_cache(maxsize=None)
def _inputs(n, H, W):
    """seeded chunk [B, n, C, H, W] and dew [B, n, L, H, W] (numpy float32) with PATTERNS planted at the first and the
    last cell of planes; computed once, shared, never written"""
    chunk = (seeded(900 + n, B, n, C, H, W) * 50).numpy().copy()
    dew = (seeded(950 + n, B, n, L, H, W, kind="rand") * 30).numpy().copy()
    cb, db = chunk.view(np.uint32), dew.view(np.uint32)
    for i, pat in enumerate(PATTERNS):
        cb[i % B, i % n, (5 * i) % C, 0, 0] = pat
        cb[(i + 1) % B, i % n, (5 * i + 3) % C, H - 1, W - 1] = pat
        db[i % B, i % n, i % L, 0, 0] = pat
        db[(i + 1) % B, i % n, (i + 6) % L, H - 1, W - 1] = pat
    chunk.setflags(write=False)
    dew.setflags(write=False)
    return chunk, dew


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _expected(spec, want, n_td, td_off, n, H, W, pad):
    """the whole buffer the launch must leave behind: sentinel everywhere except the addressed slots"""
    full = np.full(spec.numel(B, n_td, H, W) + pad, SENTINEL, np.uint32).view(np.float32)
    views = spec.views(full, B, n_td, H, W)
    assert list(views) == list(want)
    for name, v in views.items():
        v[:, td_off:td_off + n] = want[name]
    return full.view(np.int32)


def _encode(spec, chunk_d, dew_d, n_td, td_off, H, W, pad=64):
    from paradis_model_amd.encode import encode_chunk
    out = torch.empty(spec.numel(B, n_td, H, W) + pad, device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    encode_chunk(chunk_d, dew_d, spec, out, n_td, td_off)
    return out


@pytest.mark.parametrize("first", [True, False], ids=["first-chunk", "later-chunk"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("grid", [(8, 16), (5, 6)], ids=["8x16", "5x6"])
def test_encoder_equals_oracle_bit_for_bit(grid, n, first):
    cfg, names, levels, specs = _setup()
    H, W = grid
    chunk, dew = _inputs(n, H, W)
    chunk_d, dew_d = torch.from_numpy(chunk.copy()).cuda(), torch.from_numpy(dew.copy()).cuda()
    n_td, td_off = (n + 1, 1) if first else (n, 0)
    for keep in KEEPBITS:
        spec = specs[keep]
        want = EO.variables(cfg, names, levels, chunk, dew, keepbits=keep)
        out = _encode(spec, chunk_d, dew_d, n_td, td_off, H, W)
        again = _encode(spec, chunk_d, dew_d, n_td, td_off, H, W)
        torch.cuda.synchronize()
        got = _bits(out)
        assert np.array_equal(got, _expected(spec, want, n_td, td_off, n, H, W, 64)), keep
        assert np.array_equal(_bits(again), got)                                     # two runs, identical bits
        assert np.array_equal(_bits(chunk_d), chunk.view(np.int32))                  # the source is not written
        assert np.array_equal(_bits(dew_d), dew.view(np.int32))
        if keep in (23, None):                                                       # a copy of the bits
            v = spec.views(out.cpu().numpy(), B, n_td, H, W)
            assert np.array_equal(EO.bits(v["temperature"][:, td_off:td_off + n]),
                                  EO.bits(chunk[:, :, [names.index(f"temperature_h{l}") for l in levels]]))


def test_first_chunk_takes_the_initial_state_by_a_second_call():
    from paradis_model_amd.encode import encode_chunk
    cfg, names, levels, specs = _setup()
    H, W, n, spec = 8, 16, 3, specs[16]
    chunk, dew = _inputs(n, H, W)
    init, idew = _inputs(1, H, W)
    out = torch.empty(spec.numel(B, n + 1, H, W), device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    encode_chunk(torch.from_numpy(init.copy()).cuda(), torch.from_numpy(idew.copy()).cuda(), spec, out, n + 1, 0)
    encode_chunk(torch.from_numpy(chunk.copy()).cuda(), torch.from_numpy(dew.copy()).cuda(), spec, out, n + 1, 1)
    want = EO.variables(cfg, names, levels, chunk, dew, init=init, init_dew=idew, keepbits=16)
    assert np.array_equal(_bits(out), _expected(spec, want, n + 1, 0, n + 1, H, W, 0))


def test_partial_chunks_strided_views_and_the_scalar_path():
    from paradis_model_amd.encode import encode_chunk
    cfg, names, levels, specs = _setup()
    H, W, spec = 8, 16, specs[16]
    P = H * W
    chunk, dew = _inputs(3, H, W)
    big, dbig = torch.from_numpy(chunk.copy()).cuda(), torch.from_numpy(dew.copy()).cuda()
    # a trailing partial chunk: the dense 1-state view at the front of the storage of a larger buffer, as Forecaster.run
    part = big.view(-1)[:B * C * P].view(B, 1, C, H, W)
    dpart = dbig.view(-1)[:B * L * P].view(B, 1, L, H, W)
    want = EO.variables(cfg, names, levels, part.cpu().numpy(), dpart.cpu().numpy(), keepbits=16)
    out = _encode(spec, part, dpart, 1, 0, H, W)
    assert np.array_equal(_bits(out), _expected(spec, want, 1, 0, 1, H, W, 64))
    # two of three states: a batch stride of three states (and one state alone: a time stride nobody steps over)
    for a, b in ((1, 3), (2, 3)):
        want = EO.variables(cfg, names, levels, chunk[:, a:b], dew[:, a:b], keepbits=16)
        out = _encode(spec, big[:, a:b], dbig[:, a:b], b - a + 1, 1, H, W)
        assert np.array_equal(_bits(out), _expected(spec, want, b - a + 1, 1, b - a, H, W, 64))
    # bases 4 bytes past a 16-byte boundary take the scalar path: the same bits as the 16-byte path
    ref = _encode(spec, big, dbig, 3, 0, H, W, pad=0)
    co = torch.zeros(big.numel() + 1, device="cuda")[1:].view_as(big).copy_(big)
    do = torch.zeros(dbig.numel() + 1, device="cuda")[1:].view_as(dbig).copy_(dbig)
    oo = torch.zeros(ref.numel() + 1, device="cuda")[1:]
    assert co.data_ptr() % 16 == 4 and oo.data_ptr() % 16 == 4
    encode_chunk(co, do, spec, oo, 3, 0)
    assert np.array_equal(_bits(oo), _bits(ref))
    # a plane longer than one segment of the kernel (2048 values), with a ragged second segment
    H2, W2 = 33, 64
    c2, d2 = _inputs(1, H2, W2)
    want = EO.variables(cfg, names, levels, c2, d2, keepbits=16)
    out = _encode(spec, torch.from_numpy(c2.copy()).cuda(), torch.from_numpy(d2.copy()).cuda(), 2, 1, H2, W2)
    assert np.array_equal(_bits(out), _expected(spec, want, 2, 1, 1, H2, W2, 64))
    # a spec without the dew point ignores the dew chunk; host-side refusals
    nodew = type(spec).from_config(cfg, names, levels, dewpoint=False)
    want = EO.variables(cfg, names, levels, chunk, None, keepbits=16, dewpoint=False)
    out = _encode(nodew, big, None, 3, 0, H, W)
    assert np.array_equal(_bits(out), _expected(nodew, want, 3, 0, 3, H, W, 64))
    small = torch.empty(spec.numel(B, 3, H, W) - 1, device="cuda")
    with pytest.raises(ValueError, match="elements"):
        encode_chunk(big, dbig, spec, small, 3, 0)
    with pytest.raises(ValueError, match="slots"):
        encode_chunk(big, dbig, spec, ref, 3, 1)
    with pytest.raises(ValueError, match="dew"):
        encode_chunk(big, None, spec, ref, 3, 0)
    with pytest.raises(ValueError, match="dense"):
        encode_chunk(big[..., ::2], dbig, spec, ref, 3, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_chunk(big.cpu(), dbig, spec, ref, 3, 0)


# ---------------------------------------------------------------------------------- the initial state
def _post_spec(names, levels, **kw):
    from paradis_model_amd.forecast import PostSpec
    mean, std = FO.channel_stats(names, 501)
    _, _, zs = FO.classes(names, True)
    return PostSpec.from_features(names, levels, zscore_mean=mean[zs], zscore_std=std[zs], q_min=FO.Q_MIN,
                                  q_max=FO.Q_MAX, custom_normalization=True, **kw)


def _dataset(g, rec, lat, lon):
    from paradis_model_amd.dataset import DeviceDataset, DeviceStore
    cfg = default_config()
    T, H, W = g["T"], rec["H"], rec["W"]
    features = rec["features"]
    store = EO.raw_store(rec["seed"] + 10, features, T, H, W)
    times = np.datetime64("2000-02-27T00", "us") + np.arange(T) * np.timedelta64(6, "h")
    F = len(features)
    stats = {"mean": np.zeros(F, np.float32), "std": np.ones(F, np.float32), "min": np.full(F, 1e-6, np.float32),
             "max": np.full(F, 0.03, np.float32)}
    ds = DeviceStore(store.numpy(), times, features, stats, torch.from_numpy(lat), torch.from_numpy(lon),
                     seeded(7, H, W, 10), 251.3, 302.7, device="cuda")
    first = g["base"] + g["n_time_inputs"] - 1
    return store, DeviceDataset(ds, cfg, str(times[first].astype("datetime64[s]")), str(times[T - 1].astype("datetime64[s]")),
                                1, prediction_stage=True)


@pytest.mark.parametrize("grid", ["8x16", "9x16"])
def test_initial_state_vs_reference_golden(grid):
    from paradis_model_amd.encode import encode_chunk, initial_state
    cfg, names, levels, specs = _setup()
    g = load_golden("e1_encode.pt")
    rec = g["cases"][grid]
    H, W = rec["H"], rec["W"]
    lat, lon = FO.grid_deg(H, W, rec["poles"], np.float64)
    store, dataset = _dataset(g, rec, lat, lon)
    assert dataset.base == g["base"] and dataset.dyn_output_features == g["names"] == names
    post = _post_spec(names, levels)
    state, dew = initial_state(dataset, g["indices"], post, lat, lon)
    torch.cuda.synchronize()
    assert dataset.index_errors() == 0
    assert state.shape == (B, 1, C, H, W) and dew.shape == (B, 1, L, H, W) and state.is_cuda and dew.is_cuda
    got, gdew, want = state.cpu(), dew.cpu(), rec["init"]
    nan = [names.index(f) for f in rec["nan_channels"]]
    assert len(nan) == 14 and torch.isnan(got[:, :, nan]).all()                      # NaN planes are NaN
    winds = ("wind_x", "wind_y", "wind_z", "wind_x_10m", "wind_y_10m")
    worst = 0.0
    for c in range(C):
        if c in nan:
            continue
        if FO.base_name(names[c]) in winds:
            e = max_rel(got[:, :, c], want[:, :, c])
            worst = max(worst, e)
            assert e <= 1e-6, (names[c], e)
        else:                                                                        # a gather: the store's bits
            assert torch.equal(got[:, :, c], want[:, :, c]), names[c]
    print("initial state, worst wind max_rel vs the reference on a float64 grid: %.1e" % worst)
    # the dew point against the formula on the kernel's own q and T
    q, T = got[:, :, post.iq].numpy(), got[:, :, post.it].numpy()
    wdew = torch.from_numpy(FO.dewpoint_depression(q, T, levels))
    for l in range(L):
        e = max_rel(gdew[:, :, l], wdew[:, :, l])
        assert e <= 1e-6, (levels[l], e)
    print("initial dew point vs the reference's mhuaes3 on ITS q, T: %.1e" % max_rel(gdew, rec["dew"]))
    # rounding off: the encoded state is the state, regrouped; rounding on: the oracle's BitRound of the device's own state
    for keep in (None, 16):
        spec = specs[keep]
        out = torch.empty(spec.numel(B, 1, H, W), device="cuda")
        encode_chunk(state, dew, spec, out, 1, 0)
        want_vars = EO.variables(cfg, names, levels, got.numpy(), gdew.numpy(), keepbits=keep)
        have = spec.views(out.cpu().numpy(), B, 1, H, W)
        for name in want_vars:
            assert np.array_equal(EO.bits(have[name]), EO.bits(want_vars[name])), (keep, name)
        assert np.isnan(have["vertical_velocity"]).all() and np.isnan(have["total_precipitation_6hr"]).all()
    # the spec must be the dataset's
    with pytest.raises(ValueError, match="output features"):
        initial_state(dataset, g["indices"], _post_spec(names[::-1], levels, winds=False, dewpoint=False), lat, lon)


# ---------------------------------------------------------------------------------- end to end
def _model():
    from paradis_model_amd.model import Paradis
    rec = load_golden("g4_model_a.pt")
    v = rec["variant"]
    cfg = reduced_config(activation=v["activation"], adv_interpolation=v["adv_interpolation"],
                         coarsening_factor=v["coarsening_factor"])
    torch.manual_seed(42)
    m = Paradis(stub_datamodule(cfg), cfg, rec["lat_grid"], rec["lon_grid"])
    m.load_state_dict(rec["state"], strict=True)
    return m.cuda().eval()


class _Plain:
    def __init__(self):
        self.chunks = []

    def __call__(self, forecast, start_idx, dewpoint):                # today's hand-over, by keyword
        assert isinstance(forecast, np.ndarray) and forecast.dtype == np.float32
        self.chunks.append((start_idx, forecast.copy(), dewpoint.copy()))


class _Encoded:
    def __init__(self):
        self.chunks = []

    def __call__(self, variables, start_idx, pred_slice):
        assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in variables.values())
        self.chunks.append((start_idx, pred_slice, {k: v.copy() for k, v in variables.items()}))


def _rollout_inputs(g):
    s = g["seeds"]
    return (seeded(s[0], B, 1, 166, 16, 32).cuda(), seeded(s[1], B, g["S"], 16, 32, 10, kind="rand").cuda(),
            seeded(s[2], B, 1, 16, 32, 10).cuda())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_forecaster_delivers_the_oracles_variables(graph):
    from paradis_model_amd.encode import regions
    from paradis_model_amd.forecast import Forecaster
    cfg, names, levels, specs = _setup()
    g = load_golden("f5_forecast.pt")["rollout"]
    assert g["names"] == names and (g["S"], g["output_frequency"], g["write_every_n"]) == (5, 2, 2)
    lat, lon = FO.grid_deg(16, 32, False)
    fc = Forecaster(_model(), _post_spec(names, levels), lat, lon, output_frequency=2, write_every_n=2, graph=graph)
    inp, forc, const = _rollout_inputs(g)
    plain = _Plain()
    fc.run(inp, forc, const, plain)
    assert [(s, f.shape[1]) for s, f, _ in plain.chunks] == [(0, 2), (2, 1)]
    # without an encoder the hand-over is today's: the reference's rollout, to the bound of tests/test_hip_forecast.py
    ref = [g["chunk0"], load_golden("f5_forecast_tail.pt")["chunk1"]]
    for (_, f, d), r in zip(plain.chunks, ref):
        assert f.shape == tuple(r.shape) and d.shape == (B, f.shape[1], L, 16, 32)
        assert max_rel(torch.from_numpy(f), r) <= (1e-5 + 2e-6 if graph else 1e-5)   # (+ graphed against eager: 2e-6)
    init = seeded(61, B, 1, C, 16, 32) * 20
    init[:, :, names.index("total_precipitation_6hr")] = float("nan")
    init, idew = init.cuda(), (seeded(62, B, 1, L, 16, 32) * 9).cuda()
    spec = specs[16]
    pos = np.arange(4)
    for given in ((init, idew), None):
        enc = _Encoded()
        fc.run(inp, forc, const, enc, encoder=spec, init=given)
        assert len(enc.chunks) == 2
        for i, ((start, sl, got), (pstart, f, d)) in enumerate(zip(enc.chunks, plain.chunks)):
            n = f.shape[1]
            with_init = given is not None and i == 0
            want = EO.variables(cfg, names, levels, f, d, init=init.cpu().numpy() if with_init else None,
                                init_dew=idew.cpu().numpy() if with_init else None, keepbits=16)
            assert start == pstart and list(got) == list(want)
            for name in want:
                assert got[name].shape == want[name].shape, name
                assert np.array_equal(EO.bits(got[name]), EO.bits(want[name])), (graph, given is not None, i, name)
            if given is not None:                                    # the reference's regions: the init state is slot 0
                (r,) = regions([1, 0], pos, start, n)
                (w,) = EO.regions([1, 0], pos, start, n)
                assert sl == r.prediction_timedelta == slice(*w[2]) and r.rows.tolist() == w[0] == [1, 0]
                assert got["temperature"].shape[1] == sl.stop - sl.start
            else:
                assert sl == slice(1 + start, 1 + start + n) and got["temperature"].shape[1] == n
    assert [c[1] for c in enc.chunks] == [slice(1, 3), slice(3, 4)]
    # the plain hand-over is untouched by the encoded runs in between
    again = _Plain()
    fc.run(inp, forc, const, again)
    for (s0, f0, d0), (s1, f1, d1) in zip(plain.chunks, again.chunks):
        assert s0 == s1 and np.array_equal(EO.bits(f0), EO.bits(f1)) and np.array_equal(EO.bits(d0), EO.bits(d1))


def test_forecaster_refuses_a_mismatched_encoder_before_the_rollout():
    from paradis_model_amd.encode import EncodeSpec
    from paradis_model_amd.forecast import Forecaster
    cfg, names, levels, specs = _setup()
    lat, lon = FO.grid_deg(16, 32, False)

    class Never(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the rollout started")

    g = load_golden("f5_forecast.pt")["rollout"]
    inp, forc, const = _rollout_inputs(g)
    post = _post_spec(names, levels)
    fc = Forecaster(Never(), post, lat, lon, graph=False)
    other = EncodeSpec.from_config(cfg, names[1:] + names[:1], levels)
    with pytest.raises(ValueError, match="names"):
        fc.run(inp, forc, const, None, encoder=other)
    nodew = Forecaster(Never(), post, lat, lon, graph=False, dewpoint=False)
    with pytest.raises(ValueError, match="dew"):
        nodew.run(inp, forc, const, None, encoder=specs[16])
    with pytest.raises(ValueError, match="init"):
        fc.run(inp, forc, const, None, init=(torch.zeros(B, 1, C, 16, 32, device="cuda"), None))
    with pytest.raises(ValueError, match="init"):
        fc.run(inp, forc, const, None, encoder=specs[16],
               init=(torch.zeros(B, 2, C, 16, 32, device="cuda"), torch.zeros(B, 1, L, 16, 32, device="cuda")))
    with pytest.raises(ValueError, match="init"):
        fc.run(inp, forc, const, None, encoder=specs[16], init=(torch.zeros(B, 1, C, 16, 32, device="cuda"), None))
    # a spec without the dew point runs on a forecaster without it (nothing to refuse): checked up to the first step
    with pytest.raises(AssertionError, match="rollout started"):
        nodew.run(inp, forc, const, None, encoder=EncodeSpec.from_config(cfg, names, levels, dewpoint=False))
