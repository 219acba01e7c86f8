"""GPU: the forecast path (row f5) - ``paradis_forecast_post`` against the reference's own post-processing outputs
(golden f5_post.pt), the predict loop ``forecast.Forecaster`` against the reference model driven through the restated
``predict_step`` (golden f5_forecast.pt), its HIP-graph form against the eager one, and ``harness.GraphedForward``.

Bounds.  De-normalisation is the fp32 arithmetic of ``feed.normalize_features_`` (tests/test_hip_feed.py:75-82):
z-score 1e-6, humidity / precipitation 2e-5 (exp amplifies the ulp of its argument).  Winds are float64 expressions of
the fp32 de-normalised values rounded once: 1e-6 against the reference on a float64 grid, plus the reference's own
float32-grid / float64-grid spread (formed from the two goldens) against its float32-grid result.  The rollout holds
the north-star output bound 1e-5 on every stored step; the graphed rollout equals the eager one within 2e-6
(tests/test_hip_graph.py:110)."""
import time

import numpy as np
import pytest
import torch

from paradis_model_amd.config import reduced_config, stub_datamodule
from tests import forecast_oracle as FO
from tests._util import assert_chk, load_golden, max_rel, seeded

pytestmark = pytest.mark.gpu


def _spec(g, custom, **kw):
    from paradis_model_amd.forecast import PostSpec
    names = g["names"]
    mean, std = FO.channel_stats(names, g["stats_seed"])
    _, _, zs = FO.classes(names, custom)
    return PostSpec.from_features(names, g["levels"], zscore_mean=mean[zs], zscore_std=std[zs], q_min=FO.Q_MIN,
                                  q_max=FO.Q_MAX, custom_normalization=custom, **kw)


@pytest.mark.parametrize("grid", ["8x16", "9x16"])
@pytest.mark.parametrize("custom", [True, False])
@pytest.mark.parametrize("grid_dtype", ["f32", "f64"])
def test_postprocess_vs_reference_golden(grid, custom, grid_dtype):
    from paradis_model_amd import feed
    from paradis_model_amd.forecast import postprocess
    g = load_golden("f5_post.pt")
    rec, names, levels = g["cases"][grid], g["names"], g["levels"]
    H, W, C, L = rec["H"], rec["W"], len(names), len(levels)
    spec = _spec(g, custom)
    x = FO.normalised_state(rec["seed"], names, 2, 1, C, H, W)[:, 0].contiguous()
    assert_chk([x], rec["chk"])
    lat, lon = FO.grid_deg(H, W, rec["poles"], np.float32 if grid_dtype == "f32" else np.float64)
    xd = x.cuda()
    fill, dfill = seeded(11, 2, 2, C, H, W), seeded(12, 2, 2, L, H, W)
    chunk, dew = fill.cuda(), dfill.cuda()
    postprocess(xd, spec, lat, lon, chunk, 1, dew)
    torch.cuda.synchronize()
    chunk, dew = chunk.cpu(), dew.cpu()
    assert torch.equal(xd.cpu(), x)                                   # the input is what the rollout feeds back
    assert torch.equal(chunk[:, 0], fill[:, 0]) and torch.equal(dew[:, 0], dfill[:, 0])
    got = chunk[:, 1]
    want64, want32 = rec[f"custom{int(custom)}_f64"], rec[f"custom{int(custom)}_f32"]
    worst = {}
    for c in range(C):
        bound = 2e-5 if spec.kind[c] in (feed.KIND_HUMIDITY, feed.KIND_PRECIP) else 1e-6
        e64, e32 = max_rel(got[:, c], want64[:, c]), max_rel(got[:, c], want32[:, c])
        spread = max_rel(want32[:, c], want64[:, c])
        key = FO.base_name(names[c])
        worst[key] = max(worst.get(key, 0.0), e64)
        assert e64 <= bound, (names[c], e64)
        assert e32 <= bound + spread, (names[c], e32, spread)
    print("worst max_rel vs float64-grid golden per variable:", {k: f"{v:.1e}" for k, v in worst.items()})
    # dew point against the formula applied to the kernel's own de-normalised q and T
    q = got[:, spec.iq].numpy()
    T = got[:, spec.it].numpy()
    want = torch.from_numpy(FO.dewpoint_depression(q, T, levels))
    for l in range(L):
        e = max_rel(dew[:, 1, l], want[:, l])
        assert e <= 1e-6, (levels[l], e)
    if grid_dtype == "f64":
        print("dew point vs the reference's mhuaes3 on ITS q, T: %.1e" % max_rel(dew[:, 1], rec[f"dew_custom{int(custom)}"]))


def test_scalar_fallback_equals_vector_path_bit_for_bit():
    from paradis_model_amd.forecast import postprocess
    g = load_golden("f5_post.pt")
    rec, names, levels = g["cases"]["9x16"], g["names"], g["levels"]
    H, W, C, L = rec["H"], rec["W"], len(names), len(levels)
    spec = _spec(g, True)
    lat, lon = FO.grid_deg(H, W, True)
    x = FO.normalised_state(rec["seed"], names, 2, 1, C, H, W)[:, 0].contiguous().cuda()

    def run(xin, lon_, chunk, dew):
        postprocess(xin, spec, lat, lon_, chunk, 1, dew)
        return chunk[:, 1].clone(), dew[:, 1].clone()

    ref, dref = run(x, lon, torch.zeros(2, 2, C, H, W, device="cuda"), torch.zeros(2, 2, L, H, W, device="cuda"))
    # planes that start 4 bytes past a 16-byte boundary: views into flat buffers, offset by one element
    n, nd = 2 * C * H * W, 2 * 2 * L * H * W
    xo = torch.zeros(n + 1, device="cuda")[1:].view(2, C, H, W).copy_(x)
    co = torch.zeros(2 * n + 1, device="cuda")[1:].view(2, 2, C, H, W)
    do = torch.zeros(nd + 1, device="cuda")[1:].view(2, 2, L, H, W)
    assert xo.data_ptr() % 16 == 4 and co.data_ptr() % 16 == 4
    got, dgot = run(xo, lon, co, do)
    assert torch.equal(got, ref) and torch.equal(dgot, dref)
    # W % 4 != 0: the first 15 longitudes
    got, dgot = run(x[..., :15].contiguous(), lon[:15], torch.zeros(2, 2, C, H, 15, device="cuda"),
                    torch.zeros(2, 2, L, H, 15, device="cuda"))
    assert torch.equal(got, ref[..., :15]) and torch.equal(dgot, dref[..., :15])
    # a channel slice of a wider tensor (batch stride != C*H*W) is consumed in place, on the vector path
    wide = torch.zeros(2, C + 3, H, W, device="cuda")
    wide[:, :C] = x
    got, dgot = run(wide[:, :C], lon, torch.zeros(2, 2, C, H, W, device="cuda"), torch.zeros(2, 2, L, H, W, device="cuda"))
    assert torch.equal(got, ref) and torch.equal(dgot, dref)
    # without the dew-point output the state is the same
    chunk = torch.zeros(2, 2, C, H, W, device="cuda")
    postprocess(x, spec, lat, lon, chunk, 1)
    assert torch.equal(chunk[:, 1], ref)
    with pytest.raises(ValueError):
        postprocess(x, spec, lat, lon[:8], chunk, 1)
    with pytest.raises(ValueError):
        postprocess(x, spec, lat, lon, chunk, 2)


def _model(state=None):
    from paradis_model_amd.model import Paradis
    rec = load_golden("g4_model_a.pt")
    v = rec["variant"]
    cfg = reduced_config(activation=v["activation"], adv_interpolation=v["adv_interpolation"],
                         coarsening_factor=v["coarsening_factor"])
    torch.manual_seed(42)
    m = Paradis(stub_datamodule(cfg), cfg, rec["lat_grid"], rec["lon_grid"])
    m.load_state_dict(rec["state"] if state is None else state, strict=True)
    return m.cuda().eval()


def _inputs(seeds, B=2, S=5, H=16, W=32):
    return (seeded(seeds[0], B, 1, 166, H, W).cuda(), seeded(seeds[1], B, S, H, W, 10, kind="rand").cuda(),
            seeded(seeds[2], B, 1, H, W, 10).cuda())


class _Collect:
    def __init__(self):
        self.chunks = []

    def __call__(self, forecast, start_idx, dewpoint):
        assert isinstance(forecast, np.ndarray) and forecast.dtype == np.float32
        self.chunks.append((start_idx, torch.from_numpy(forecast.copy()),
                            None if dewpoint is None else torch.from_numpy(dewpoint.copy())))


def _forecaster(model, g, graph):
    from paradis_model_amd.forecast import Forecaster
    lat, lon = FO.grid_deg(16, 32, False)
    return Forecaster(model, _spec(g, True), lat, lon, output_frequency=g["output_frequency"],
                      write_every_n=g["write_every_n"], graph=graph)


def _per_channel(a, b):
    return max(max_rel(a[:, :, c], b[:, :, c]) for c in range(a.shape[2]))


@pytest.mark.parametrize("gemm", ["bf16x3", "exact"])
def test_forecaster_eager_vs_reference_rollout(gemm, monkeypatch):
    """values <= 1e-5 on every stored step (the north-star output bound): over the whole state and per channel"""
    from paradis_model_amd import feed, ops
    monkeypatch.setattr(ops, "GEMM_SCHEME", ops._SCHEMES[gemm])
    g = load_golden("f5_forecast.pt")["rollout"]
    want = [g["chunk0"], load_golden("f5_forecast_tail.pt")["chunk1"]]
    inp, forc, const = _inputs(g["seeds"], g["B"], g["S"])
    assert_chk([inp.cpu(), forc.cpu(), const.cpu()], g["chk"])
    fc = _forecaster(_model(), g, graph=False)
    col = _Collect()
    fc.run(inp, forc, const, col)
    assert len(col.chunks) == g["n_chunks"] and [c[0] for c in col.chunks] == g["start_idx"]
    for (start, got, dew), ref in zip(col.chunks, want):
        assert got.shape == ref.shape and dew.shape == (ref.shape[0], ref.shape[1], 13, 16, 32)
        for t in range(ref.shape[1]):
            e = max_rel(got[:, t], ref[:, t])
            per = [max_rel(got[:, t, c], ref[:, t, c]) for c in range(ref.shape[2])]
            hum = [c for c in range(ref.shape[2]) if fc.spec.kind[c] == feed.KIND_HUMIDITY]
            print("stored step %d: max_rel %.2e, worst channel %.2e (%s), worst humidity channel %.2e" % (
                start + t, e, max(per), g["names"][int(np.argmax(per))], max(per[c] for c in hum)))
            assert e <= 1e-5
            for c, ec in enumerate(per):
                assert ec <= 1e-5, (start + t, g["names"][c], ec)
        assert torch.isfinite(dew).all() and float(dew.max()) <= 30.0


def test_forecaster_graph_equals_eager_and_follows_the_weights():
    g = load_golden("f5_forecast.pt")["rollout"]
    model = _model()
    eager, graphed = _forecaster(model, g, False), _forecaster(model, g, True)
    runs = []
    for seeds in ((177, 179, 180), (277, 279, 280)):
        inp, forc, const = _inputs(seeds)
        a, b = _Collect(), _Collect()
        eager.run(inp, forc, const, a)
        graphed.run(inp, forc, const, b)
        assert [c[0] for c in a.chunks] == [c[0] for c in b.chunks] == [0, 2]
        for (_, x, dx), (_, y, dy) in zip(a.chunks, b.chunks):
            assert x.shape == y.shape and _per_channel(y, x) <= 2e-6 and _per_channel(dy, dx) <= 2e-6
        runs.append(b.chunks)
    assert len(graphed._steps) == 1                                   # one capture for both runs
    assert max_rel(runs[1][0][1], runs[0][0][1]) > 1e-5                # different inputs, different forecasts
    # parameters written in place are honoured by the next replay without re-capture
    torch.manual_seed(9)
    sd = {k: (v + 0.05 * v.abs().mean() * torch.randn_like(v) if v.is_floating_point() else v)
          for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    c = _Collect()
    graphed.run(inp, forc, const, c)
    assert len(graphed._steps) == 1
    fresh = _Collect()
    _forecaster(_model(sd), g, False).run(inp, forc, const, fresh)
    for (_, x, _), (_, y, _), (_, z, _) in zip(fresh.chunks, c.chunks, runs[1]):
        assert _per_channel(y, x) <= 2e-6
        assert max_rel(y, z) > 1e-5


def test_forecaster_under_inference_mode_and_chunking_corners():
    g = load_golden("f5_forecast.pt")["rollout"]
    from paradis_model_amd.forecast import Forecaster
    model = _model()
    lat, lon = FO.grid_deg(16, 32, False)
    spec = _spec(g, True)
    inp, forc, const = _inputs((177, 179, 180))
    base = _Collect()
    Forecaster(model, spec, lat, lon, graph=False).run(inp, forc, const, base)       # one chunk of 5 states
    assert len(base.chunks) == 1 and base.chunks[0][1].shape == (2, 5, 97, 16, 32)
    for graph in (False, True):
        with torch.inference_mode():
            i2, f2, c2 = inp.clone(), forc.clone(), const.clone()                     # inference tensors
            fc = Forecaster(model, spec, lat, lon, write_every_n=2, graph=graph)
            col = _Collect()
            fc.run(i2, f2, c2, col)
        col2 = _Collect()
        fc.run(inp, forc, const, col2)                                               # and again outside the mode
        for got in (col, col2):
            assert [c[0] for c in got.chunks] == [0, 2, 4] and [c[1].shape[1] for c in got.chunks] == [2, 2, 1]
            whole = torch.cat([c[1] for c in got.chunks], dim=1)
            assert _per_channel(whole, base.chunks[0][1]) <= 2e-6
            dwhole = torch.cat([c[2] for c in got.chunks], dim=1)
            assert _per_channel(dwhole, base.chunks[0][2]) <= 2e-6


def test_graphed_forward_under_inference_mode():
    from paradis_model_amd.harness import GraphedForward
    model = _model()
    x = [seeded(31 + i, 2, 186, 16, 32).cuda() for i in range(2)]
    with torch.inference_mode():
        gf = GraphedForward(model, x[0])
        for xi in x:
            y = gf(xi).clone()
            assert max_rel(y, model(xi)) <= 2e-6
    with torch.no_grad():
        assert max_rel(gf(x[0]), model(x[0])) <= 2e-6
    assert max_rel(gf(x[1]), y) == 0.0                                 # the static output is overwritten by each call


def test_graphed_forecast_host_time():
    """what the graph buys: per-step host time of run(graph=True) against run(graph=False), nothing synchronised inside
    the timed loop (no hand-over: on_chunk=None)"""
    from paradis_model_amd.forecast import Forecaster
    g = load_golden("f5_forecast.pt")["rollout"]
    model = _model()
    lat, lon = FO.grid_deg(16, 32, False)
    S = 16
    inp, forc, const = _inputs((177, 179, 180), S=S)
    t = {}
    for graph in (False, True):
        fc = Forecaster(model, _spec(g, True), lat, lon, output_frequency=4, write_every_n=2, graph=graph)
        fc.run(inp, forc, const, lambda **kw: None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fc.run(inp, forc, const, None)
        t[graph] = (time.perf_counter() - t0) / (3 * S)
        torch.cuda.synchronize()
    print("host time per forecast step: eager %.2f ms, graph replay %.2f ms" % (1e3 * t[False], 1e3 * t[True]))
    assert t[True] < 0.5 * t[False]
