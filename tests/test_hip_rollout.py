"""GPU: the two pieces the no-grad loops share (paradis_model_amd/rollout.py) - the chunk hand-over ring on its own, with
no model, and the launches ``Forecaster.run`` issues through it, counted against the chunk plan."""
import numpy as np
import pytest
import torch

from tests import forecast_oracle as FO
from tests._util import load_golden

pytestmark = pytest.mark.gpu


def test_chunk_ring_hand_over():
    """five chunks of a [1, 2, 1, 2, 4] pair, the last one partial: every chunk arrives once, in order, with its own
    values, one flush late, and the two pinned tensors take turns"""
    from paradis_model_amd.rollout import ChunkRing
    sizes = [2, 2, 2, 2, 1]

    def run(receive):
        ring = ChunkRing("cuda", {"state": (1, 2, 1, 2, 4)}).pin()
        got, flushed = [], [0]

        def on_chunk(start, n, host):
            a = host["state"].numpy()
            got.append((start, a.copy(), n, flushed[0], host["state"].untyped_storage().data_ptr()))

        fn = on_chunk if receive else None
        for i, n in enumerate(sizes):
            view = ring.open(n)["state"]
            assert view.shape == (1, n, 1, 2, 4)
            view.fill_(float(i + 1))
            ring.flush((2 * i, n))
            flushed[0] += 1
            ring.deliver(fn)
        ring.deliver(fn, keep=0)
        assert not ring.pending
        return got

    got = run(True)
    assert [g[0] for g in got] == [0, 2, 4, 6, 8]                                # five deliveries, in order
    for i, (start, a, n, flushed, ptr) in enumerate(got):
        assert n == sizes[i] and a.shape == (1, n, 1, 2, 4) and a.dtype == np.float32
        assert np.array_equal(a, np.full((1, n, 1, 2, 4), i + 1, np.float32))
        assert flushed == min(i + 2, len(sizes))              # chunk i: after flush of chunk i+1 returned (the last: at the end)
    ptrs = [g[4] for g in got]
    assert all(ptrs[i] != ptrs[i + 1] for i in range(4)) and all(ptrs[i] == ptrs[i + 2] for i in range(3))
    assert run(False) == []                                                      # no receiver: returns, nothing delivered
    torch.cuda.synchronize()


def _model():
    from paradis_model_amd.config import reduced_config, stub_datamodule
    from paradis_model_amd.model import Paradis
    rec = load_golden("g4_model_a.pt")
    v = rec["variant"]
    cfg = reduced_config(activation=v["activation"], adv_interpolation=v["adv_interpolation"],
                         coarsening_factor=v["coarsening_factor"])
    torch.manual_seed(42)
    m = Paradis(stub_datamodule(cfg), cfg, rec["lat_grid"], rec["lon_grid"])
    m.load_state_dict(rec["state"], strict=True)
    return m.cuda().eval()


def test_forecaster_launch_counts():
    """B = 2, S = 5, every step stored, chunks of 2: 5 stored states in 3 chunks.  The plan gives the launches: one
    post-processing per stored state (two with a model-space truth) and one score per stored state; one encode per
    chunk, plus one for the initial state in the first chunk."""
    from paradis_model_amd import _lib
    from paradis_model_amd.config import default_config
    from paradis_model_amd.encode import EncodeSpec
    from paradis_model_amd.forecast import Forecaster, PostSpec
    from paradis_model_amd.verify import Scorecard
    from tests._util import seeded
    g = load_golden("f5_forecast.pt")["rollout"]
    names, levels = g["names"], list(default_config().features.pressure_levels)
    B, S, H, W, C, L = 2, 5, 16, 32, len(names), len(levels)
    mean, std = FO.channel_stats(names, g["stats_seed"])
    _, _, zs = FO.classes(names, True)
    spec = PostSpec.from_features(names, levels, zscore_mean=mean[zs], zscore_std=std[zs], q_min=FO.Q_MIN,
                                  q_max=FO.Q_MAX, custom_normalization=True)
    lat, lon = FO.grid_deg(H, W, False)
    inputs = (seeded(177, B, 1, 166, H, W).cuda(), seeded(179, B, S, H, W, 10, kind="rand").cuda(),
              seeded(180, B, 1, H, W, 10).cuda())
    truth = FO.normalised_state(31, names, B, S, C, H, W).cuda()
    encoder = EncodeSpec.from_config(default_config(), names, levels)
    init = (torch.zeros(B, 1, C, H, W, device="cuda"), torch.zeros(B, 1, L, H, W, device="cuda"))
    model = _model()
    want = {"plain": (5, 0, 0), "scorecard": (10, 5, 0), "encoder+init": (5, 0, 4), "encoder": (5, 0, 3)}
    for graph in (False, True):
        fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=graph)
        card = Scorecard(names, torch.ones(H), S)
        runs = {"plain": {}, "scorecard": dict(scorecard=card, truth=truth, truth_normalized=True),
                "encoder+init": dict(encoder=encoder, init=init), "encoder": dict(encoder=encoder)}
        fc.run(*inputs, None)                        # capture and lazy tables, outside the counted runs
        for name, kw in runs.items():
            chunks = []
            prof = _lib.LaunchProfiler()
            _lib.PROFILER = prof
            try:
                fc.run(*inputs, lambda **k: chunks.append(k["start_idx"]), **kw)
            finally:
                _lib.PROFILER = None
            assert chunks == [0, 2, 4], (graph, name)
            got = tuple(len(prof.records.get(k, (0, ()))[1]) for k in ("forecast_post", "verify_update", "forecast_encode"))
            assert got == want[name], (graph, name, got)
