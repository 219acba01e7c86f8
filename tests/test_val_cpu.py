"""CPU: the validation path's host side - ``validate.ReportSpec`` tables against the branch the reference's
``_get_report_rmse`` took for each feature (golden v1_val.pt), argument rejection of ``paradis_val_score`` before any
HIP call, the "no CPU fallback" refusals, and tests/val_oracle.py in fp32 against the reference's own numbers."""
import ctypes

import numpy as np
import pytest
import torch

from tests import forecast_oracle as FO
from tests import val_oracle as VO
from tests._util import assert_chk, load_golden


@pytest.fixture(scope="module")
def G():
    return load_golden("v1_val.pt")


def _spec(G, feats, custom, **kw):
    from paradis_model_amd.validate import ReportSpec
    return ReportSpec.from_features(feats, G["names"], report_std=VO.report_std(G["names"], feats, G["stats_seed"]),
                                    custom_normalization=custom, q_min=G["q_min"], q_max=G["q_max"], **kw)


@pytest.mark.parametrize("custom", [True, False])
def test_reportspec_tables_match_reference_branches(G, custom):
    from paradis_model_amd import feed
    from paradis_model_amd.config import default_config, feature_layout
    from paradis_model_amd.validate import ReportSpec
    s = G["single"]
    feats, names = s["features"], G["names"]
    # a humidity level feature, total_precipitation_6hr, two z-score features, a duplicate
    assert feats == VO.SINGLE_REPORTS and feats[0] == feats[4] and "specific_humidity_h850" in feats
    assert names == feature_layout(default_config()).output_name_order
    spec = _spec(G, feats, custom)
    assert spec.names == feats and spec.num_reports == 5
    assert spec.chan.tolist() == s["indices"]
    codes = {"zscore": feed.KIND_ZSCORE, "humidity": feed.KIND_HUMIDITY, "precipitation": feed.KIND_PRECIP}
    for grid in ("8x16", "9x16"):
        br = s["cases"][grid][f"branches_custom{int(custom)}"]
        assert spec.cls.tolist() == [codes[b] for b in br]
    assert set(spec.cls.tolist()) == ({1, 2, 3} if custom else {1})
    for r, f in enumerate(feats):
        if spec.cls[r] == feed.KIND_ZSCORE:
            assert spec.p1[r] == np.float32(s["std"][r])               # report_std is indexed by report position
        elif spec.cls[r] == feed.KIND_HUMIDITY:
            assert (spec.p0[r], spec.p1[r]) == (np.float32(G["q_min"]), np.float32(G["q_max"]))
    # the default feature list is the output name order
    d = ReportSpec.from_features(feats, report_std=s["std"], custom_normalization=custom, q_min=1e-7, q_max=0.025)
    assert d.chan.tolist() == s["indices"]
    # the same tuples the oracle uses
    want = VO.report_tuples(names, feats, custom, s["std"])
    assert [(int(c), int(k)) for c, k in zip(spec.chan, spec.cls)] == [(t[0], t[1]) for t in want]
    # the rollout's list
    ro = G["rollout"]
    rs = _spec(G, ro["features"], True)
    assert rs.chan.tolist() == ro["indices"] and rs.cls.tolist() == [codes[b] for b in ro["branches"]]


def test_reportspec_corners(G):
    from paradis_model_amd.validate import ReportSpec, row_size
    names = G["names"]
    empty = ReportSpec.from_features([], names, report_std=[], custom_normalization=True)
    assert empty.num_reports == 0 and empty.chan.size == 0 and row_size(97, 0) == 195
    with pytest.raises(ValueError):
        ReportSpec.from_features(["no_such_feature"], names, report_std=[1.0], custom_normalization=True)
    with pytest.raises(ValueError):                                   # one std per report feature
        ReportSpec.from_features(["2m_temperature"], names, report_std=[1.0, 2.0], custom_normalization=False)
    with pytest.raises(ValueError):                                   # humidity branch without its constants
        ReportSpec.from_features(["specific_humidity_h850"], names, report_std=[1.0], custom_normalization=True)
    with pytest.raises(ValueError):                                   # one channel, two different standard deviations
        ReportSpec.from_features(["2m_temperature"] * 2, names, report_std=[1.0, 2.0], custom_normalization=True)
    # substring tests as the reference writes them, in its order: humidity first
    odd = ["specific_humidity_precipitation", "my_precipitation", "plain"]
    sp = ReportSpec.from_features(odd, odd, report_std=[1.0, 2.0, 3.0], custom_normalization=True, q_min=1e-7, q_max=0.02)
    assert sp.cls.tolist() == [2, 3, 1] and sp.chan.tolist() == [0, 1, 2]
    sp = ReportSpec.from_features(odd, odd, report_std=[1.0, 2.0, 3.0], custom_normalization=False)
    assert sp.cls.tolist() == [1, 1, 1] and sp.p1.tolist() == [1.0, 2.0, 3.0]


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_val_score_rejects_bad_arguments_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    assert "paradis_val_score" in _lib.SIGNATURES and "paradis_val_score_ws_bytes" in _lib.SIGNATURES
    assert L.paradis_abi_version() == 10
    S = 97 * 128
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first (or has B == 0)

    def call(kind=1, chan=(), cls=(), lat=None, B=0, C=97, H=8, W=16, pbs=S, tbs=S):
        R = len(chan)
        ch = ctypes.cast(_ints(*chan), ctypes.c_void_p) if R else None
        cl = ctypes.cast(_ints(*cls), ctypes.c_void_p) if R else None
        dev = fake if R else None
        return L.paradis_val_score(None, pbs, None, tbs, None, None, lat, kind, 1.0, ch, cl, R, dev, dev, dev, dev, dev,
                                   None, None, B, C, H, W, None)

    assert call() == 0                                               # B == 0: accepted, nothing to do
    assert call(kind=2) == 0 and call(kind=0) == 0
    assert call(chan=(7, 7), cls=(1, 1), lat=fake) == 0              # a duplicate report channel is fine
    for bad in (3, -1):
        assert call(kind=bad) == 1 and "kind" in _lib.last_error()
    assert call(chan=(97,), cls=(1,), lat=fake) == 1 and "channel" in _lib.last_error()
    assert call(chan=(-1,), cls=(1,), lat=fake) == 1 and "channel" in _lib.last_error()
    for bad in (0, 4):
        assert call(chan=(3,), cls=(bad,), lat=fake) == 1 and "class" in _lib.last_error()
    assert call(chan=(3,), cls=(2,), lat=None) == 1 and "latitude" in _lib.last_error()
    for kw in (dict(B=-1), dict(C=-1), dict(H=-8), dict(W=-16), dict(C=0)):
        assert call(**kw) == 1 and "shape" in _lib.last_error()
    assert call(pbs=S - 1) == 1 and "stride" in _lib.last_error()
    assert call(tbs=10) == 1 and "stride" in _lib.last_error()
    assert call(B=2) == 1 and "null" in _lib.last_error()            # B > 0 without tensors
    # the workspace: three partials per workgroup, one workgroup per piece of 8192 cells of every plane
    assert L.paradis_val_score_ws_bytes(2, 97, 8, 16) == 3 * 97 * 2 * 4
    assert L.paradis_val_score_ws_bytes(1, 5, 100, 200) == 3 * 5 * 3 * 4
    assert L.paradis_val_score_ws_bytes(0, 97, 8, 16) == 0 and L.paradis_val_score_ws_bytes(-1, 97, 8, 16) == 0


def test_score_and_validator_refuse_cpu_tensors(G):
    from paradis_model_amd.config import default_config
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.validate import Validator, score
    lat_deg = torch.from_numpy(FO.grid_deg(8, 16, False, np.float32)[0])
    loss = build_loss(default_config(), lat_deg)
    spec = _spec(G, VO.ROLLOUT_REPORTS, True)
    x = torch.zeros(2, 97, 8, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        score(x, x, loss, spec, torch.zeros(1 + 2 * 97 + 3))
    batch = (torch.zeros(2, 1, 166, 8, 16), torch.zeros(2, 1, 97, 8, 16), torch.zeros(2, 1, 8, 16, 10),
             torch.zeros(2, 1, 8, 16, 10))
    v = Validator(lambda mi: mi[:, :97], loss, spec)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.step(batch)
    with pytest.raises(RuntimeError):
        v.result()                                                    # nothing scored


def _loss_tables(lat_deg, kind, latw):
    from paradis_model_amd.config import default_config
    from paradis_model_amd.loss import build_loss
    cfg = default_config()
    cfg.training.loss_function.type = kind
    cfg.training.loss_function.lat_weights = latw
    fn = build_loss(cfg, lat_deg)
    return fn.feature_weights, fn.lat_weights, float(fn.delta)


@pytest.mark.parametrize("grid", ["8x16", "9x16"])
@pytest.mark.parametrize("custom", [True, False])
def test_oracle_fp32_reproduces_reference_numbers(G, grid, custom):
    s = G["single"]
    rec, names, feats = s["cases"][grid], G["names"], s["features"]
    pred, tgt = VO.single_state(rec["seed"], names, 2, rec["H"], rec["W"])
    assert pred.shape == (2, 97, rec["H"], rec["W"])
    assert_chk([pred, tgt], rec["chk"])
    reports = VO.report_tuples(names, feats, custom, s["std"])
    worst = 0.0
    for kind in ("reversed_huber", "mse"):
        for latw in (True, False):
            wf, lat_w, delta = _loss_tables(rec["lat_deg"], kind, latw)
            assert delta == rec["delta"]
            want = rec["rows"][(custom, kind, latw)]
            got = VO.row(pred, tgt, wf, lat_w if latw else None, lat_w, kind, delta, reports, dtype=torch.float32)
            assert got.dtype == torch.float32 and got.shape == want.shape == (1 + 2 * 97 + 5,)
            err = ((got.double() - want.double()).abs() / want.double().abs().clamp_min(1e-30)).max()
            worst = max(worst, float(err))
            assert float(err) <= 1e-6, (kind, latw, float(err))
            # the fp64 evaluation agrees with the reference's fp32 numbers at fp32 level
            r64 = VO.row(pred, tgt, wf, lat_w if latw else None, lat_w, kind, delta, reports)
            assert float(((r64 - want.double()).abs() / want.double().abs()).max()) <= 1e-5
            assert float(got[1 + 2 * 97]) == float(got[1 + 2 * 97 + 4])            # the duplicate
    print(f"fp32 oracle vs the reference's numbers, worst relative difference: {worst:.2e}")


def test_rollout_golden_is_consistent(G):
    ro = G["rollout"]
    n = 1 + 2 * 97 + 3
    assert ro["rows"].shape == (3, n) and ro["grad_l1"].shape == (3, n) and ro["ymax"].shape == (3,)
    assert float(ro["grad_l1"].min()) >= 0 and float(ro["grad_l1"][:, 0].min()) > 0
    assert abs(float(ro["val_loss"]) - float(ro["rows"][:, 0].mean())) <= 1e-6 * float(ro["val_loss"])
    assert torch.allclose(ro["reports"], ro["rows"][:, -3:].mean(0), rtol=1e-6, atol=0)
    assert ro["features"] == VO.ROLLOUT_REPORTS and ro["loss_kind"] == "reversed_huber" and ro["lat_weights"]
