"""CPU: forecast verification without a device - the fp64 oracle (tests/verify_oracle.py) against closed forms, the
C-ABI symbols of ``csrc/verify.hip`` and their argument rejection before any HIP call, the workspace layout, and the
host side of ``verify.Scorecard`` (argument errors, ``result`` arithmetic, ``table``) and of
``Forecaster.run(scorecard=...)``."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import verify_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("paradis_verify_piece", "paradis_verify_ws_bytes", "paradis_verify_update")
H, W = 4, 8
LATW = torch.tensor([1.0, 2.0, 3.0, 2.0])


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _one(f, t, clim=True):
    """scores of one update at lead 0 with a zero climatology"""
    C = f.shape[1]
    cl = torch.zeros(1, C, H, W, dtype=torch.float64) if clim else None
    return VO.scores([(0, f, t, None)], LATW, 1, C, clim=cl)


# ================================================================================================ 1. the oracle
def test_oracle_identical_fields():
    t = _rand(1, 3, 2, H, W)
    acc, r = _one(t.clone(), t)
    assert (r["rmse"] == 0).all() and (r["bias"] == 0).all() and (r["mae"] == 0).all()
    assert np.allclose(r["acc"], 1.0, rtol=0, atol=1e-15) and np.allclose(r["activity"], 1.0, rtol=0, atol=1e-15)
    assert r["count"].tolist() == [3.0] and (acc[0, :, 5] == 3).all()


@pytest.mark.parametrize("d", [0.75, -2.5])
def test_oracle_constant_offset(d):
    t = _rand(2, 2, 3, H, W)
    _, r = _one(t + d, t)
    assert np.allclose(r["bias"], d, rtol=1e-14) and np.allclose(r["rmse"], abs(d), rtol=1e-14)
    assert np.allclose(r["mae"], abs(d), rtol=1e-14)


def test_oracle_anticorrelated_and_doubled_anomalies():
    t = _rand(3, 2, 2, H, W)
    _, r = _one(-t, t)
    assert np.allclose(r["acc"], -1.0, rtol=0, atol=1e-15) and np.allclose(r["activity"], 1.0, rtol=0, atol=1e-15)
    _, r = _one(2 * t, t)
    assert np.allclose(r["acc"], 1.0, rtol=0, atol=1e-15) and np.allclose(r["activity"], 2.0, rtol=0, atol=1e-15)
    # with a climatology that is not zero the anomalies, not the fields, are what is compared
    cl = _rand(4, 1, 2, H, W) + 7.0
    ta = _rand(5, 2, 2, H, W)
    _, r = VO.scores([(0, cl - ta, cl + ta, None)], LATW, 1, 2, clim=cl)
    assert np.allclose(r["acc"], -1.0, rtol=0, atol=1e-13)
    _, base = VO.scores([(0, ta, 0 * ta, None)], LATW, 1, 2)                 # f - t = -2 ta
    assert np.allclose(r["rmse"] ** 2, 4 * base["rmse"] ** 2, rtol=1e-13)


@pytest.mark.parametrize("row", [0, 2, 3])
def test_oracle_error_confined_to_one_row(row):
    t = _rand(6, 1, 2, H, W)
    e = _rand(7, 1, 2, W)
    f = t.clone()
    f[:, :, row] += e
    _, r = _one(f, t)
    want = float(LATW[row]) * e.square().mean(-1)[0].numpy() / float(LATW.sum())
    assert np.allclose(r["rmse"][0] ** 2, want, rtol=1e-13)
    assert np.allclose(r["bias"][0], float(LATW[row]) * e.mean(-1)[0].numpy() / float(LATW.sum()), rtol=1e-12)


def test_oracle_sample_without_truth_anomaly_is_left_out_of_acc_only():
    t = _rand(8, 3, 2, H, W)
    t[1] = 0.0
    f = t + 0.5 * _rand(9, 3, 2, H, W)
    acc, r = _one(f, t)
    assert (acc[0, :, 0] == 3).all() and (acc[0, :, 5] == 2).all()
    _, rest = _one(f[[0, 2]], t[[0, 2]])
    assert np.allclose(r["acc"], rest["acc"], rtol=1e-14)
    _, alone = _one(f[1:2], t[1:2])
    assert np.isnan(alone["acc"]).all() and (alone["rmse"] > 0).all()
    assert np.allclose(3 * r["rmse"] ** 2, 2 * rest["rmse"] ** 2 + alone["rmse"] ** 2, rtol=1e-13)


def test_oracle_without_climatology_leads_and_fp32_variant():
    t, n = _rand(10, 2, 2, H, W), _rand(11, 2, 2, H, W)
    acc, r = VO.scores([(1, t + n, t, None)], LATW, 3, 2)
    assert np.isnan(r["acc"]).all() and np.isnan(r["activity"]).all()
    assert r["count"].tolist() == [0.0, 2.0, 0.0]
    assert np.isnan(r["rmse"][0]).all() and np.isnan(r["rmse"][2]).all() and np.isfinite(r["rmse"][1]).all()
    assert (acc[1, :, 4:] == 0).all()
    for seq in (False, True):
        _, r32 = VO.scores([(1, (t + n).float(), t.float(), None)], LATW, 3, 2, dtype=torch.float32, seq=seq)
        _, r64 = VO.scores([(1, (t + n).float(), t.float(), None)], LATW, 3, 2)
        for k in ("rmse", "bias", "mae"):
            e = np.abs(r32[k][1] - r64[k][1]).max() / np.abs(r64[k][1]).max()
            assert 0 <= e < 1e-5, (k, e)


# ================================================================================================ 2.-4. the C ABI
def test_verify_symbols_are_declared_exported_and_bound():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    sig = _lib.SIGNATURES["paradis_verify_update"][1]
    assert len(sig) == 16 and sig[8] is ctypes.c_double and sig[1] is ctypes.c_int64 and sig[3] is ctypes.c_int64
    assert _lib.SIGNATURES["paradis_verify_ws_bytes"][0] is ctypes.c_size_t
    assert _lib.lib.paradis_abi_version() == 10
    piece = _lib.lib.paradis_verify_piece()
    assert piece >= 1024 and piece % 1024 == 0


def test_verify_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first

    def call(fc=fake, truth=fake, clim=None, idx=None, K=0, lat=fake, Z=1.0, acc=fake, ws=fake, B=2, C=3, H=4, W=8,
             fc_bs=96, truth_bs=96):
        return L.paradis_verify_update(fc, fc_bs, truth, truth_bs, clim, idx, K, lat, Z, acc, ws, B, C, H, W, None)

    assert call(clim=fake, K=1) == 1 and "clim_index" in _lib.last_error()
    assert call(idx=fake, K=1) == 1 and "clim_index" in _lib.last_error()
    for kw in (dict(C=0), dict(H=0), dict(W=0), dict(C=-1), dict(B=-1)):
        assert call(**kw) == 1 and "shape" in _lib.last_error(), kw
    for K in (0, -3):
        assert call(clim=fake, idx=fake, K=K) == 1 and "K must be" in _lib.last_error()
    for Z in (0.0, -1.0, float("nan"), float("inf")):
        assert call(Z=Z) == 1 and "Z must be" in _lib.last_error(), Z
        assert call(Z=Z, B=0) == 1 and "Z must be" in _lib.last_error(), Z
    assert call(acc=None) == 1 and "acc" in _lib.last_error()
    assert call(ws=None) == 1 and "ws" in _lib.last_error()
    assert call(B=2 ** 20, C=2 ** 12, fc_bs=2 ** 20, truth_bs=2 ** 20) == 1 and "grid" in _lib.last_error()
    assert call(fc_bs=95) == 1 and "stride" in _lib.last_error()
    # B == 0: nothing to do, whatever the pointers
    assert L.paradis_verify_update(None, 0, None, 0, None, None, 0, None, 1.0, None, None, 0, 3, 4, 8, None) == 0


def test_verify_workspace_layout():
    """double [6 with a climatology, else 3][B*C][ceil(H*W / piece)]"""
    from paradis_model_amd import _lib
    L = _lib.lib
    piece = L.paradis_verify_piece()
    for (B, C, Hh, Ww) in ((3, 5, 9, 30), (1, 97, 721, 1440)):
        npieces = -(-(Hh * Ww) // piece)
        assert L.paradis_verify_ws_bytes(B, C, Hh, Ww, 1) == 6 * B * C * npieces * 8
        assert L.paradis_verify_ws_bytes(B, C, Hh, Ww, 0) == 3 * B * C * npieces * 8
    assert L.paradis_verify_ws_bytes(1, 1, 1, piece + 1, 0) == 3 * 2 * 8
    assert L.paradis_verify_ws_bytes(0, 5, 9, 30, 1) == 0 and L.paradis_verify_ws_bytes(1, 0, 9, 30, 1) == 0


# ================================================================================================ 5. host logic
NAMES = ["t2m", "z500", "q850"]


def _card(**kw):
    from paradis_model_amd.verify import Scorecard
    return Scorecard(NAMES, LATW, 3, device="cpu", **kw)


def test_scorecard_constructor_errors():
    from paradis_model_amd.verify import Scorecard
    with pytest.raises(ValueError, match="names"):
        Scorecard([], LATW, 3, device="cpu")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_leads"):
            Scorecard(NAMES, LATW, bad, device="cpu")
    for bad in (torch.zeros(4), torch.tensor([1.0, -1.0, 1.0, 1.0]), torch.tensor([1.0, float("nan"), 1.0, 1.0])):
        with pytest.raises(ValueError, match="lat_weights"):
            Scorecard(NAMES, bad, 3, device="cpu")
    for bad in (torch.zeros(2, 3, H, W, dtype=torch.float64), torch.zeros(2, 2, H, W), torch.zeros(2, 3, H + 1, W),
                torch.zeros(3, H, W)):
        with pytest.raises(ValueError, match="climatology"):
            Scorecard(NAMES, LATW, 3, device="cpu", climatology=bad)
    card = _card(climatology=torch.zeros(2, 3, H, W))
    assert card.acc.shape == (3, 3, 8) and card.acc.dtype == torch.float64 and card.n_leads == 3
    loss = type("L", (), {"lat_weights_buf": LATW.view(1, 1, -1, 1)})()
    assert Scorecard.lat_weights_from(loss) is loss.lat_weights_buf
    assert Scorecard(NAMES, Scorecard.lat_weights_from(loss), 1, device="cpu").lat_w.tolist() == LATW.tolist()


def test_scorecard_update_argument_errors_on_cpu_tensors():
    f = torch.zeros(2, 3, H, W)
    card = _card()
    for lead in (-1, 3, 1.0, None):
        with pytest.raises(ValueError, match="lead"):
            card.update(lead, f, f)
    with pytest.raises(ValueError, match="forecast"):
        card.update(0, f.double(), f)
    with pytest.raises(ValueError, match="truth"):
        card.update(0, f, f.double())
    with pytest.raises(ValueError, match="forecast"):
        card.update(0, torch.zeros(2, 4, H, W), torch.zeros(2, 4, H, W))
    with pytest.raises(ValueError, match="forecast"):
        card.update(0, f[0], f[0])
    with pytest.raises(ValueError, match="truth"):
        card.update(0, f, torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="forecast"):
        card.update(0, torch.zeros(2, 3, H, 2 * W)[..., ::2], f)
    with pytest.raises(ValueError, match="truth"):
        card.update(0, f, torch.zeros(2, 3, W, H).transpose(-1, -2))
    with pytest.raises(ValueError, match="clim_index"):
        card.update(0, f, f, torch.zeros(2, dtype=torch.int32))
    with_clim = _card(climatology=torch.zeros(2, 3, H, W))
    with pytest.raises(ValueError, match="clim_index"):
        with_clim.update(0, f, f)                                   # two slots: the index is needed
    with pytest.raises(ValueError, match="clim_index"):
        with_clim.update(0, f, f, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="clim_index"):
        with_clim.update(0, f, f, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="climatology"):
        with_clim.update(0, torch.zeros(2, 3, H, W + 4), torch.zeros(2, 3, H, W + 4), torch.zeros(2, dtype=torch.int32))
    # valid arguments on the CPU: there is no CPU fallback
    with pytest.raises(RuntimeError, match="MI355X"):
        card.update(0, f, f)
    assert (card.acc == 0).all()


def test_scorecard_result_arithmetic_from_a_hand_filled_accumulator():
    card = _card(climatology=torch.zeros(1, 3, H, W))
    #                       n   se    e    ae  acc_b n_acc  ff    tt
    card.acc[0, 0] = torch.tensor([4.0, 16.0, -2.0, 6.0, 1.5, 3.0, 8.0, 32.0], dtype=torch.float64)
    card.acc[0, 1] = torch.tensor([4.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    card.acc[0, 2] = torch.tensor([4.0, 0.0, 0.0, 0.0, -4.0, 4.0, 9.0, 1.0], dtype=torch.float64)
    card.acc[2] = card.acc[0] * 2
    r = card.result()
    assert r["names"] == NAMES and r["count"].tolist() == [4.0, 0.0, 8.0]
    for k in ("rmse", "bias", "mae", "acc", "activity"):
        assert r[k].shape == (3, 3) and r[k].dtype == np.float64
        assert np.isnan(r[k][1]).all(), k                                      # the lead never updated
    assert r["rmse"][0].tolist() == [2.0, 0.5, 0.0] and r["bias"][0].tolist() == [-0.5, 0.25, 0.0]
    assert r["mae"][0].tolist() == [1.5, 0.25, 0.0]
    assert r["acc"][0][0] == 0.5 and math.isnan(r["acc"][0][1]) and r["acc"][0][2] == -1.0
    assert r["activity"][0][0] == 0.5 and math.isnan(r["activity"][0][1]) and r["activity"][0][2] == 3.0
    assert r["rmse"][2].tolist() == r["rmse"][0].tolist() and r["acc"][2][0] == 0.5
    want = VO.report(card.acc, True)
    for k in ("rmse", "bias", "mae", "acc", "activity", "count"):
        assert np.array_equal(r[k], want[k], equal_nan=True), k
    # without a climatology acc and activity are NaN whatever the accumulator holds
    plain = _card()
    plain.acc.copy_(card.acc)
    r2 = plain.result(sync_dist=True)                                          # no process group: a plain read
    assert np.isnan(r2["acc"]).all() and np.isnan(r2["activity"]).all()
    assert np.array_equal(r2["rmse"], r["rmse"], equal_nan=True)
    plain.reset()
    assert (plain.acc == 0).all() and np.isnan(plain.result()["rmse"]).all() and plain.result()["count"].tolist() == [0, 0, 0]


def test_scorecard_result_sync_dist_makes_one_all_reduce(tmp_path, monkeypatch):
    """with a process group ``result(sync_dist=True)`` sums ``acc`` over the ranks by ONE all-reduce (here: one gloo
    rank, so the sum is the rank's own) and leaves the accumulators as they were"""
    import torch.distributed as dist
    card = _card(climatology=torch.zeros(1, 3, H, W))
    card.acc[1] = torch.arange(1.0, 25.0, dtype=torch.float64).view(3, 8)
    want = card.result()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        calls = []
        real = dist.all_reduce
        monkeypatch.setattr(dist, "all_reduce", lambda t, **kw: (calls.append(tuple(t.shape)), real(t, **kw))[1])
        keep = card.acc.clone()
        got = card.result(sync_dist=True)
        assert calls == [(3, 3, 8)] and torch.equal(card.acc, keep)
        assert card.result() is not None and len(calls) == 1                  # no collective without sync_dist
    finally:
        dist.destroy_process_group()
    for k in ("rmse", "bias", "mae", "acc", "activity", "count"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_scorecard_table_formatting():
    from paradis_model_amd.verify import Scorecard
    card = _card(climatology=torch.zeros(1, 3, H, W))
    card.acc[0, :, 0] = 2.0
    card.acc[0, :, 1] = torch.tensor([8.0, 18.0, 32.0], dtype=torch.float64)
    r = card.result()
    text = Scorecard.table(r)
    lines = text.split("\n")
    blocks = text.split("\n\n")
    assert len(blocks) == 5 and [b.split()[0] for b in blocks] == ["rmse", "bias", "mae", "acc", "activity"]
    assert lines[0].split() == ["rmse", "count"] + NAMES
    assert lines[1].split() == ["0", "2", "2.0000e+00", "3.0000e+00", "4.0000e+00"]
    assert lines[2].split() == ["1", "0", "nan", "nan", "nan"]
    assert all(len(b.split("\n")) == 4 for b in blocks)
    assert len({len(line) for line in blocks[0].split("\n")}) == 1               # aligned columns
    sub = Scorecard.table(r, channels=["q850", "t2m"])
    assert sub.split("\n")[0].split() == ["rmse", "count", "q850", "t2m"]
    assert sub.split("\n")[1].split() == ["0", "2", "4.0000e+00", "2.0000e+00"]
    with pytest.raises(ValueError, match="nope"):
        Scorecard.table(r, channels=["nope"])


# ================================================================================================ 6. the forecaster hook
def test_forecaster_run_refuses_a_scorecard_without_truth():
    from paradis_model_amd.forecast import Forecaster, PostSpec
    spec = PostSpec.from_features(NAMES, [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    fc = Forecaster(None, spec, np.zeros(H), np.zeros(W), graph=False)
    inp, forc, const = torch.zeros(1, 1, 6, H, W), torch.zeros(1, 2, H, W, 1), torch.zeros(1, 1, H, W, 1)
    with pytest.raises(ValueError, match="truth"):
        fc.run(inp, forc, const, None, scorecard=_card(), truth=None)
