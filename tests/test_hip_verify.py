"""GPU: forecast verification - the kernel pair ``paradis_verify_update`` through ``verify.Scorecard`` against plain fp64
(tests/verify_oracle.py) at its dispatch edges, its closed forms, its bit-level promises (vector path == scalar path,
run == run, two updates == one update of the concatenated batch), and the ``Forecaster.run(scorecard=...)`` hook.

Protocol of the edge cases: that of tests/test_hip_kernel_edges.py (the ``_Judge`` below restates its helper).  Per
metric vector (``[C]`` values of one lead) e = max|x - ref64| / max|ref64| for the kernel (e_hip) and for the oracle's
fp32 variant (e_cpu: the larger of ATen's float32 plane sum and a strictly sequential float32 sum).  Asserted: the
project's forward ceiling e_hip <= 1e-5 and e_hip <= 1.5 e_cpu + 1e-7; both figures are printed and recorded.

Input design.  truth = clim[k[b]] + a, forecast = truth + offset_c + sigma noise with a, noise ~ N(0, 1), sigma = 0.6
and |offset_c| in [0.7, 1.1] with alternating sign (>= sigma: the bias does not cancel); so the anomalies correlate and
the per-sample ACC lies in roughly 0.3 .. 0.95.  The first and last cell of every plane and the last cell in front of
each piece boundary carry 2^10 times the anomaly and the error of the rest (fixed values of alternating sign, so that
the few cells that dominate the squared sums keep the ACC in range): a cell dropped or counted twice there moves every
sum by far more than any bound.  In the all-positive case every value of f, t, clim and f - t is > 0.  Every
design is checked with the fp64 oracle on the CPU before the kernel is judged on it: every metric vector has
max|ref| > 0, no sample is left out of the ACC mean, the per-sample ACC lies in [0.25, 0.97].

Shapes come from ``paradis_verify_piece()`` (PIECE below): a plane is cut into ceil(H W / PIECE) pieces, one workgroup
each; 16-byte loads iff W % 4 == 0 and every plane base is 16-byte aligned, else scalar loads."""
import functools

import numpy as np
import pytest
import torch

from tests import forecast_oracle as FO
from tests import verify_oracle as VO
from tests._util import make_grid, seeded

pytestmark = pytest.mark.gpu
FWD = 1e-5
SPIKE = 1024.0
SIGMA = 0.6


@functools.lru_cache(None)
def _piece():
    from paradis_model_amd import _lib
    return int(_lib.lib.paradis_verify_piece())


def _e(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


class _Judge:
    """collects e_hip / e_cpu per metric vector, prints and records them, asserts both bounds at the end
    (tests/test_hip_kernel_edges.py; ``yardstick=False``: the ceiling only)"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad = record_property, case, []

    def add(self, name, got, ref, cpu, ceil, seq=None, yardstick=True):
        e_hip, e_cpu = _e(got, ref), _e(cpu, ref)
        if seq is not None:
            e_cpu = max(e_cpu, _e(seq, ref))
        print(f"VERIFY | {self.case} | {name} | e_hip {e_hip:.2e} | e_cpu {e_cpu:.2e}")
        self.rp(name, f"e_hip={e_hip:.3e} e_cpu={e_cpu:.3e}")
        if not e_hip <= ceil:
            self.bad.append((name, "ceiling", e_hip, ceil))
        if yardstick and not e_hip <= 1.5 * e_cpu + 1e-7:
            self.bad.append((name, "fp32 yardstick", e_hip, e_cpu))

    def done(self):
        assert not self.bad, (self.case, self.bad)


# ================================================================================================ inputs
def lat_weights(H):
    """cos(latitude) of an equiangular grid without pole rows, normalised to mean 1 (fp32)"""
    lat = (-90.0 + 90.0 / H + (180.0 / H) * np.arange(H)) * np.pi / 180.0
    w = np.cos(lat)
    return torch.from_numpy((w / w.mean()).astype(np.float32))


def spike_cells(P, piece):
    return sorted({0, P - 1} | {j * piece - 1 for j in range(1, (P - 1) // piece + 1)})


def design(seed, B, C, H, W, K, piece, positive=False):
    """(forecast, truth [B, C, H, W], clim [K, C, H, W], k [B] int32) fp32 on the CPU, by the module docstring"""
    P = H * W
    a = seeded(seed, B, C, P)
    noise = seeded(seed + 1, B, C, P)
    off = torch.tensor([(0.7 + 0.1 * (c % 5)) * (1.0 if positive or c % 2 == 0 else -1.0) for c in range(C)])
    if positive:
        a, noise = a.abs() + 0.05, noise.abs()
    err = off.view(1, C, 1) + SIGMA * noise
    for j, cell in enumerate(spike_cells(P, piece)):          # deterministic spikes: they dominate the squared sums
        sign = 1.0 if positive or j % 2 == 0 else -1.0
        size = (0.4 if j % 2 == 0 else 1.6) if positive else 1.0
        wiggle = 0.5 * (1.0 if j % 2 == 0 else -1.0)
        a[..., cell] = SPIKE * sign * size
        err[..., cell] = SPIKE * (off.view(1, C) + SIGMA * wiggle)
    clim = 3.0 * seeded(seed + 2, K, C, P)
    if positive:
        clim = clim.abs() + 1.0
    k = torch.tensor([(b + 1) % K for b in range(B)], dtype=torch.int32)
    truth = clim[k.long()] + a
    fc = truth + err
    if positive:
        assert (fc > 0).all() and (truth > 0).all() and (clim > 0).all() and (fc - truth > 0).all()
    return fc.view(B, C, H, W), truth.view(B, C, H, W), clim.view(K, C, H, W), k


def check_design(fc, truth, clim, k, w):
    """the fp64 oracle on the inputs, before they are relied on: nothing cancels, nothing is left out"""
    sums = VO.plane_sums(fc, truth, w, clim, k)
    acc_b = sums[5] / torch.sqrt(sums[3] * sums[4])
    assert ((sums[3] * sums[4]) != 0).all()
    assert 0.25 <= float(acc_b.min()) and float(acc_b.max()) <= 0.97, (float(acc_b.min()), float(acc_b.max()))
    assert float((sums[1].abs() / sums[2]).min()) >= 0.5            # |sum w d| against sum w |d|: the bias does not cancel
    return acc_b


# name -> (B, C, H, W as functions of the piece size, layout, with climatology (K = 2), all-positive)
#   layout "dense": contiguous tensors;  "offset": the forecast is a view one float past a 16-byte boundary (scalar path
#   at W % 4 == 0);  "views": forecast = chunk[:, 1] of [B, 3, C, H, W], truth = true[:, 1] of [B, 2, C, H, W]
def _cases(piece):
    rows = piece // 128
    return {
        "9x30 P<piece W%4!=0":            (3, 5, 9, 30, "dense", True, False),
        "9x30 views no-clim":             (3, 5, 9, 30, "views", False, False),
        "9x30 all-positive":              (3, 5, 9, 30, "dense", True, True),
        "P==piece":                       (1, 5, rows, 128, "dense", True, False),
        "P=piece+W":                      (3, 1, rows + 1, 128, "dense", True, False),
        "P=piece+W offset (scalar)":      (3, 5, rows + 1, 128, "offset", True, False),
        "P=piece+W views (vector)":       (3, 5, rows + 1, 128, "views", True, False),
        "P=piece+H W%4!=0 across pieces": (1, 1, rows, 129, "dense", True, False),
        "P=piece+W no-clim B=1":          (1, 5, rows + 1, 128, "dense", False, False),
    }


CASE_NAMES = list(_cases(8192))          # the names do not depend on the piece size


def place(fc, truth, layout):
    """device tensors holding ``fc`` / ``truth`` in the memory layout of the case"""
    B, C, H, W = fc.shape
    if layout == "dense":
        return fc.cuda(), truth.cuda()
    if layout == "offset":
        f = torch.zeros(fc.numel() + 1, device="cuda")[1:].view(B, C, H, W)
        f.copy_(fc)
        assert f.data_ptr() % 16 == 4
        return f, truth.cuda()
    chunk = torch.full((B, 3, C, H, W), float("nan"), device="cuda")
    true = torch.full((B, 2, C, H, W), float("nan"), device="cuda")
    chunk[:, 1] = fc.cuda()
    true[:, 1] = truth.cuda()
    f, t = chunk[:, 1], true[:, 1]
    assert f.stride(0) != t.stride(0) and f.stride(0) != C * H * W
    return f, t


def judge_result(J, tag, got, updates, w, n_leads, C, clim):
    """every metric vector of every updated lead against the fp64 oracle, with the fp32 yardsticks"""
    _, r64 = VO.scores(updates, w, n_leads, C, clim=clim)
    _, r32 = VO.scores(updates, w, n_leads, C, clim=clim, dtype=torch.float32)
    _, rseq = VO.scores(updates, w, n_leads, C, clim=clim, dtype=torch.float32, seq=True)
    assert np.array_equal(got["count"], r64["count"])
    for lead in sorted({u[0] for u in updates}):
        for m in (VO.METRICS if clim is not None else ("rmse", "bias", "mae")):
            assert np.abs(r64[m][lead]).max() > 0, (m, lead)
            J.add(f"{tag}{m}[{lead}]", got[m][lead], r64[m][lead], r32[m][lead], FWD, seq=rseq[m][lead])
    if clim is None:
        assert np.isnan(got["acc"]).all() and np.isnan(got["activity"]).all()
    return r64


# ================================================================================================ 1. the kernel pair
@pytest.mark.parametrize("case", CASE_NAMES)
def test_update_at_dispatch_edges(case, record_property):
    from paradis_model_amd.verify import Scorecard
    piece = _piece()
    B, C, H, W, layout, with_clim, positive = _cases(piece)[case]
    fc, truth, clim, k = design(100 + CASE_NAMES.index(case), B, C, H, W, 2, piece, positive)
    w = lat_weights(H)
    acc_b = check_design(fc, truth, clim, k, w)
    print(f"VERIFY | {case} | P = {H * W} = {H * W // piece} pieces + {H * W % piece} cells | per-sample ACC "
          f"{float(acc_b.min()):.3f} .. {float(acc_b.max()):.3f}")
    names = [f"c{i}" for i in range(C)]
    card = Scorecard(names, w, 2, climatology=clim.cuda() if with_clim else None)
    f, t = place(fc, truth, layout)
    before = (f.clone(), t.clone())
    card.update(1, f, t, k.cuda() if with_clim else None)
    got = card.result()
    assert torch.equal(f, before[0]) and torch.equal(t, before[1])            # neither input is written
    assert got["names"] == names and got["count"].tolist() == [0.0, float(B)]
    assert all(np.isnan(got[m][0]).all() for m in VO.METRICS)                 # the lead never updated
    acc = card.acc.cpu()
    assert (acc[0] == 0).all() and (acc[1, :, 0] == B).all()
    assert (acc[1, :, 5] == (B if with_clim else 0)).all()
    J = _Judge(record_property, case)
    judge_result(J, "", got, [(1, fc, truth, k)], w, 2, C, clim if with_clim else None)
    J.done()


@pytest.mark.parametrize("H,W,weights", [(4, 8, [1.0, 2.0, 3.0, 2.0]),              # 16-byte loads
                                         (5, 6, [1.0, 2.0, 3.0, 2.0, 5.0])])        # quads that straddle two rows
def test_closed_forms_on_the_device(H, W, weights):
    from paradis_model_amd.verify import Scorecard
    C = 2
    w = torch.tensor(weights)
    g = torch.Generator().manual_seed(5)
    t = torch.round(torch.randn(3, C, H, W, generator=g) * 64) / 64              # exact sums and differences in fp32
    t[t == 0] = 1 / 64
    zero = torch.zeros(1, C, H, W, device="cuda")

    def run(f, t_):
        card = Scorecard(["a", "b"], w, 1, climatology=zero)
        card.update(0, f.cuda().contiguous(), t_.cuda().contiguous())
        return card.result(), card.acc.cpu()[0]

    r, _ = run(t.clone(), t)
    assert (r["rmse"] == 0).all() and (r["bias"] == 0).all() and (r["mae"] == 0).all()
    assert np.abs(r["acc"] - 1).max() <= 1e-15 and np.abs(r["activity"] - 1).max() <= 1e-15
    for d in (0.75, -2.5):
        r, _ = run(t + d, t)
        assert np.abs(r["bias"] - d).max() <= 1e-6 * abs(d) and np.abs(r["rmse"] - abs(d)).max() <= 1e-6 * abs(d)
        assert np.abs(r["mae"] - abs(d)).max() <= 1e-6 * abs(d)
    r, _ = run(-t, t)
    assert np.abs(r["acc"] + 1).max() <= 1e-15 and np.abs(r["activity"] - 1).max() <= 1e-15
    r, _ = run(2 * t, t)
    assert np.abs(r["acc"] - 1).max() <= 1e-15 and np.abs(r["activity"] - 2).max() <= 1e-15
    for row in range(H):
        e = torch.round(torch.randn(1, C, W, generator=g) * 16) / 16
        f = t[:1].clone()
        f[:, :, row] += e
        r, _ = run(f, t[:1])
        want = float(w[row]) * e.double().square().mean(-1)[0].numpy() / float(w.sum())
        assert np.abs(r["rmse"][0] ** 2 - want).max() <= 1e-6 * want.max(), row
    t0 = t.clone()
    t0[1] = 0.0                                        # a sample without a truth anomaly: out of acc, kept in rmse
    f0 = t0 + 0.5
    r, acc = run(f0, t0)
    assert acc[:, 0].tolist() == [3.0, 3.0] and acc[:, 5].tolist() == [2.0, 2.0]
    assert np.abs(r["rmse"] - 0.5).max() <= 1e-6
    _, ref = VO.scores([(0, f0, t0, None)], w, 1, C, clim=zero.cpu())
    assert np.abs(r["acc"] - ref["acc"]).max() <= 1e-6


def test_bit_level_promises():
    """vector path == scalar path, run == run, two updates == one update of the concatenated batch (bit for bit), and
    the concatenated batch against the oracle; B == 0 and reset()"""
    from paradis_model_amd.verify import Scorecard
    piece = _piece()
    B, C, H, W = 3, 5, piece // 128 + 1, 128
    fc, truth, clim, k = design(300, B, C, H, W, 2, piece)
    w = lat_weights(H)
    names = [f"c{i}" for i in range(C)]
    climd, kd = clim.cuda(), k.cuda()

    def fresh():
        return Scorecard(names, w, 2, climatology=climd)

    fv, tv = place(fc, truth, "dense")
    fs, ts = place(fc, truth, "offset")
    a, b, c = fresh(), fresh(), fresh()
    a.update(0, fv, tv, kd)
    b.update(0, fs, ts, kd)
    c.update(0, fv, tv, kd)
    assert torch.equal(a.acc, b.acc), "the scalar path and the vector path differ"
    assert torch.equal(a.acc, c.acc), "two runs differ"
    assert float(a.acc[0].abs().min()) > 0 and (a.acc[1] == 0).all()
    # without a climatology the two paths agree as well, and fields 4 .. 7 stay untouched
    p, q = Scorecard(names, w, 2), Scorecard(names, w, 2)
    p.acc.fill_(7.0)
    q.acc.fill_(7.0)
    p.update(1, fv, tv)
    q.update(1, fs, ts)
    assert torch.equal(p.acc, q.acc) and (p.acc[1, :, 4:] == 7).all() and (p.acc[0] == 7).all()
    # two updates on one lead == one update of the concatenated batch
    two = fresh()
    two.update(0, fv[:2], tv[:2], kd[:2])
    two.update(0, fv[2:], tv[2:], kd[2:])
    assert torch.equal(two.acc, a.acc)
    got = two.result()
    _, ref = VO.scores([(0, fc[:2], truth[:2], k[:2]), (0, fc[2:], truth[2:], k[2:])], w, 2, C, clim=clim)
    _, whole = VO.scores([(0, fc, truth, k)], w, 2, C, clim=clim)
    for m in VO.METRICS:
        assert np.array_equal(ref[m][0], whole[m][0]) and _e(got[m][0], whole[m][0]) <= FWD, m
    # B == 0 leaves the accumulators untouched
    keep = two.acc.clone()
    two.update(0, fv[:0], tv[:0], kd[:0])
    two.update(1, fv[:0], tv[:0], kd[:0])
    assert torch.equal(two.acc, keep)
    two.reset()
    assert (two.acc == 0).all() and np.isnan(two.result()["rmse"]).all()
    two.update(0, fv, tv, kd)
    assert torch.equal(two.acc, a.acc)                                  # and it counts again from zero


def test_update_refusals_on_the_device():
    from paradis_model_amd.verify import Scorecard
    w = lat_weights(4)
    card = Scorecard(["a"], w, 1, climatology=torch.zeros(2, 1, 4, 8, device="cuda"))
    f = torch.zeros(2, 1, 4, 8, device="cuda")
    with pytest.raises(ValueError, match="clim_index"):
        card.update(0, f, f, torch.zeros(2, dtype=torch.int32))              # the index must live on the device
    with pytest.raises(ValueError, match="climatology"):
        Scorecard(["a"], w, 1, climatology=torch.zeros(2, 1, 4, 8))           # and the climatology too
    # a slot out of range is not read: the sample's scores are NaN
    card.update(0, f + 1, f, torch.tensor([0, 2], dtype=torch.int32, device="cuda"))
    assert np.isnan(card.result()["rmse"]).all()


# ================================================================================================ 2. the forecaster hook
class _Collect:
    def __init__(self):
        self.chunks = []

    def __call__(self, forecast, start_idx, dewpoint):
        self.chunks.append((start_idx, torch.from_numpy(forecast.copy())))


@functools.lru_cache(None)
def _rollout_setup():
    from paradis_model_amd.config import feature_layout, reduced_config, stub_datamodule
    from paradis_model_amd.forecast import PostSpec
    from paradis_model_amd.model import Paradis
    H, W, B, S = 9, 30, 2, 3
    cfg = reduced_config()
    _, lg, og = make_grid(H, W, True)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).cuda().eval()
    names = list(feature_layout(cfg).output_name_order)
    levels = list(cfg.features.pressure_levels)
    mean, std = FO.channel_stats(names)
    _, _, zs = FO.classes(names, True)
    spec = PostSpec.from_features(names, levels, zscore_mean=mean[zs], zscore_std=std[zs], q_min=FO.Q_MIN,
                                  q_max=FO.Q_MAX, custom_normalization=True)
    lat, lon = FO.grid_deg(H, W, True)
    inputs = (seeded(177, B, 1, 166, H, W).cuda(), seeded(179, B, S, H, W, 10, kind="rand").cuda(),
              seeded(180, B, 1, H, W, 10).cuda())
    return model, spec, lat, lon, inputs, (H, W, B, S)


@pytest.mark.parametrize("truth_normalized,graph", [(False, False), (True, True)])
def test_forecaster_hook(truth_normalized, graph, record_property):
    """run(scorecard=..., truth=...) scores the chunks it hands to on_chunk: bit for bit the accumulators of a scorecard
    updated by hand with those chunks, and the fp64 oracle's values; the chunks are those of a run without a scorecard.

    Bounds against the oracle: the forward ceiling 1e-5 on every channel's own scale (each column is divided by
    max_lead |ref| of its channel, so a small-valued channel is judged as strictly as a large one) for rmse, mae and
    activity, with the fp32 yardstick.  The forecast is a model output, so its bias and ACC may cancel: their absolute
    error is held against the magnitude of the summands - |bias error| <= 1e-5 mae, |acc error| <= 1e-5 (sqrt(ff tt)
    bounds |ft|) - which is what an fp32 sum can promise."""
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.verify import Scorecard
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    C = spec.num_channels
    w = lat_weights(H)
    # truth and climatology: seeded normalised states, taken to physical units by the package's own post-processing
    norm = FO.normalised_state(31, spec.names, B, S, C, H, W).cuda()
    phys = torch.empty(B, S, C, H, W, device="cuda")
    clim = torch.empty(1, 2, C, H, W, device="cuda")
    cnorm = FO.normalised_state(32, spec.names, 1, 2, C, H, W).cuda()
    for s in range(S):
        postprocess(norm[:, s], spec, lat, lon, phys, s)
    for s in range(2):
        postprocess(cnorm[:, s], spec, lat, lon, clim, s)
    clim = clim[0].contiguous()
    kidx = torch.tensor([[0, 1, 1], [1, 0, 1]], dtype=torch.int32, device="cuda")
    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=graph)
    plain = _Collect()
    fc.run(*inputs, plain)
    card = Scorecard(spec.names, w, S, climatology=clim)
    scored = _Collect()
    fc.run(*inputs, scored, scorecard=card, truth=norm if truth_normalized else phys,
           truth_normalized=truth_normalized, clim_index=kidx)
    assert [c[0] for c in scored.chunks] == [0, 2] and [c[1].shape[1] for c in scored.chunks] == [2, 1]
    for (s0, x), (s1, y) in zip(plain.chunks, scored.chunks):
        assert s0 == s1 and torch.equal(x, y)
    states = torch.cat([c[1] for c in scored.chunks], dim=1)                   # [B, S, C, H, W] as the writer saw them
    by_hand = Scorecard(spec.names, w, S, climatology=clim)
    for s in range(S):
        by_hand.update(s, states[:, s].cuda(), phys[:, s], kidx[:, s].contiguous())
    assert torch.equal(card.acc, by_hand.acc)
    got = card.result()
    assert got["count"].tolist() == [float(B)] * S
    ups = [(s, states[:, s], phys[:, s].cpu(), kidx[:, s].cpu()) for s in range(S)]
    climc = clim.cpu()
    _, r64 = VO.scores(ups, w, S, C, clim=climc)
    _, r32 = VO.scores(ups, w, S, C, clim=climc, dtype=torch.float32)
    _, rseq = VO.scores(ups, w, S, C, clim=climc, dtype=torch.float32, seq=True)
    J = _Judge(record_property, f"hook normalized={truth_normalized} graph={graph}")
    for m in ("rmse", "mae", "activity"):
        scale = np.abs(r64[m]).max(axis=0, keepdims=True)
        assert (scale > 0).all(), m
        J.add(m, got[m] / scale, r64[m] / scale, r32[m] / scale, FWD, seq=rseq[m] / scale)
    J.done()
    assert (np.abs(got["bias"] - r64["bias"]) <= FWD * r64["mae"]).all()
    assert np.isfinite(r64["acc"]).all() and np.abs(got["acc"] - r64["acc"]).max() <= FWD
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, scorecard=card, truth=phys[:, :2])               # a wrong n_stored: before the rollout
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, scorecard=card)
    assert torch.equal(card.acc, by_hand.acc)
