"""GPU: zonal power spectra - the kernel pair ``paradis_spectrum_update`` through ``spectrum.Spectra`` against plain
fp64 (tests/spectrum_oracle.py) at its dispatch edges, its bit-level promises, the weight rules, the cross-check
against ``verify.Scorecard`` and the ``Forecaster.run(spectra=...)`` hook.

Protocol of the edge cases: the ``_Judge`` of tests/test_hip_verify.py with the norm of ``spectrum_oracle.error`` over
the accumulated sums of a lead - per (channel, band), for k >= 1 ``max_k |S - S64| / sqrt(max(S64_ff[k], S64_tt[k]) *
max(tot_ff, tot_tt))`` with ``tot = sum_{k >= 1} S64``, for k = 0 the relative error of S_ff and S_tt - for the kernel
(e_hip) and for the oracle's two float32 yardsticks with the same pivot (e_cpu: the larger of ``torch.fft.fft`` on
complex64 and a complex64 matrix DFT).  Asserted: the project's forward ceiling e_hip <= 1e-5 and e_hip <=
max(3 e_cpu, 1e-6), the rule of tests/test_hip_amse_edges.py; both figures are printed and recorded.  Every case runs
the plain design and its offset variant (1e5 added to both fields) under the same bound; a transform without the pivot
cannot meet it (tests/test_spectrum_cpu.py shows that on the CPU).

Shapes come from the exported dispatch constants: ROWS = ``paradis_spectrum_rows()`` rows of a plane per workgroup (H in
{1, ROWS - 1, ROWS, ROWS + 1, 2 ROWS + 1}), the ``fft`` schedule for W in {4, 6, 8, 30, 50, 64, 90, 256, 1440} (every
radix, one to six passes, one to ROWS rows in flight) and the ``direct`` schedule for W in {14, 26,
``paradis_spectrum_direct_max_w()``}; B in {1, 3}, C <= 3, R in {1, 3}.  The three-band cases leave the rows poleward
of 60 N without weight in any band (not transformed) and rows outside a band out of it.

Not here: the ``fft`` and ``direct`` schedules on one W.  The schedule is a function of W alone and the library has no
override; none was added for the test."""
import functools

import numpy as np
import pytest
import torch

from tests import spectrum_oracle as SO

pytestmark = pytest.mark.gpu
FWD = 1e-5
FLOOR = 1e-6
BANDS3 = {"south": (-90.0, -20.0), "tropics": (-20.0, 20.0), "north-mid": (20.0, 60.0)}


@functools.lru_cache(None)
def _consts():
    from paradis_model_amd import _lib
    L = _lib.lib
    return int(L.paradis_spectrum_rows()), int(L.paradis_spectrum_fft_max_w()), int(L.paradis_spectrum_direct_max_w())


class _Judge:
    """collects e_hip / e_cpu per accumulated lead, prints and records them, asserts both bounds at the end"""

    def __init__(self, record_property, case):
        self.rp, self.case, self.bad = record_property, case, []

    def add(self, name, got, S64, cpu):
        e_hip = SO.error(got, S64)
        e_cpu = max(SO.error(c, S64) for c in cpu)
        print(f"SPECTRUM | {self.case} | {name} | e_hip {e_hip:.2e} | e_cpu {e_cpu:.2e}")
        self.rp(name, f"e_hip={e_hip:.3e} e_cpu={e_cpu:.3e}")
        if not e_hip <= FWD:
            self.bad.append((name, "ceiling", e_hip, FWD))
        if not e_hip <= max(3.0 * e_cpu, FLOOR):
            self.bad.append((name, "fp32 yardstick", e_hip, e_cpu))

    def done(self):
        assert not self.bad, (self.case, self.bad)


def _names(C):
    return [f"c{i}" for i in range(C)]


def _spectra(C, H, n_leads, R, **kw):
    from paradis_model_amd.spectrum import Spectra
    lat, w = SO.cos_weights(H)
    return Spectra(_names(C), lat, n_leads, bands=BANDS3 if R == 3 else None, weights=torch.from_numpy(w), **kw)


def _acc64(updates, sp, n_leads, **kw):
    return SO.accumulate(updates, sp.band_w, n_leads, **kw)


# name -> (W, H as a function of ROWS, B, C, R, layout); "views": forecast = chunk[:, 1], truth = true[:, 1]
def _cases():
    rows, _, dmax = 32, 4096, 254
    try:
        rows, _, dmax = _consts()
    except Exception:           # (collection without the library: the names below do not depend on the constants)
        pass
    return {
        "fft W=4 H=1":                 (4, 1, 1, 1, 1, "dense"),
        "fft W=6 H=rows-1 R=3":        (6, rows - 1, 3, 2, 3, "dense"),
        "fft W=8 H=rows":              (8, rows, 1, 3, 1, "views"),
        "fft W=30 H=rows+1 R=3":       (30, rows + 1, 3, 2, 3, "views"),
        "fft W=50 H=2rows+1 R=3":      (50, 2 * rows + 1, 1, 2, 3, "dense"),
        "fft W=64 H=rows+1":           (64, rows + 1, 3, 3, 1, "dense"),
        "fft W=64 H=2rows+1 R=3":      (64, 2 * rows + 1, 1, 2, 3, "dense"),
        "fft W=90 H=rows R=3":         (90, rows, 1, 2, 3, "dense"),
        "fft W=256 H=rows+1":          (256, rows + 1, 1, 2, 1, "dense"),
        "fft W=1440 H=3":              (1440, 3, 1, 2, 1, "dense"),
        "fft W=1440 H=rows+1 R=3":     (1440, rows + 1, 1, 1, 3, "dense"),
        "direct W=14 H=rows+1 R=3":    (14, rows + 1, 3, 2, 3, "views"),
        "direct W=26 H=1":             (26, 1, 1, 3, 1, "dense"),
        "direct W=max H=2rows+1":      (dmax, 2 * rows + 1, 1, 2, 1, "dense"),
        "direct W=max H=rows-1 R=3":   (dmax, rows - 1, 3, 1, 3, "dense"),
    }


CASE_NAMES = list(_cases())


def place(fc, truth, layout):
    """device tensors holding ``fc`` / ``truth`` in the memory layout of the case"""
    B, C, H, W = fc.shape
    if layout == "dense":
        return fc.cuda(), truth.cuda()
    chunk = torch.full((B, 3, C, H, W), float("nan"), device="cuda")
    true = torch.full((B, 2, C, H, W), float("nan"), device="cuda")
    chunk[:, 1] = fc.cuda()
    true[:, 1] = truth.cuda()
    return chunk[:, 1], true[:, 1]


# ================================================================================================ 1. the kernel pair
@pytest.mark.parametrize("case", CASE_NAMES)
def test_update_at_dispatch_edges(case, record_property):
    from paradis_model_amd import spectrum
    W, H, B, C, R, layout = _cases()[case]
    assert spectrum.schedule(W) == case.split()[0]
    J = _Judge(record_property, case)
    for offset in (False, True):
        f, t = SO.design(500 + CASE_NAMES.index(case), B, C, H, W, offset)
        sp = _spectra(C, H, 2, R)
        assert sp.band_w.shape == (R, H) and (R == 1 or (sp.band_w.sum(0) == 0).any() or H < 6)
        if not offset:
            SO.check_design(f, t, sp.band_w)
        fd, td = place(f, t, layout)
        before = (fd.clone(), td.clone())
        sp.update(1, fd, td)
        got = sp.result()
        assert torch.equal(fd, before[0]) and torch.equal(td, before[1])            # neither input is written
        assert got["count"].tolist() == [0.0, float(B)] and got["names"] == _names(C)
        acc = sp.acc.cpu().numpy()
        assert acc.shape == (2, C, R, W // 2 + 1, 3) and (acc[0] == 0).all()
        acc64, _ = _acc64([(1, f, t)], sp, 2)
        cpu = [_acc64([(1, f, t)], sp, 2, method=m)[0][1] for m in ("fft32", "dft32")]
        J.add("offset" if offset else "plain", acc[1], acc64[1], cpu)
        want = SO.report(acc, sp.count.cpu().numpy())                                # the host arithmetic of result()
        for q in SO.QUANTITIES:
            assert np.array_equal(got[q], want[q], equal_nan=True), q
            assert np.isnan(got[q][0]).all() and np.isfinite(got[q][1]).all(), q
    J.done()


# ================================================================================================ 2. bit-level promises
@pytest.mark.parametrize("W", [30, 64, 14])
def test_bit_level_promises(W):
    """run == run, two updates == one update of the concatenated batch, a channel alone == the channel among others,
    ``channels=`` == the slice of the full result, a non-dense batch stride == its dense copy (all bit for bit);
    B == 0 and reset()"""
    rows = _consts()[0]
    B, C, H, R = 3, 3, rows + 1, 3
    f, t = SO.design(700 + W, B, C, H, W)
    fd, td = place(f, t, "dense")
    fv, tv = place(f, t, "views")
    assert fv.stride(0) != tv.stride(0) and fv.stride(0) != C * H * W

    def fresh(**kw):
        return _spectra(C, H, 2, R, **kw)

    a, b, v = fresh(), fresh(), fresh()
    a.update(0, fd, td)
    b.update(0, fd, td)
    v.update(0, fv, tv)
    assert torch.equal(a.acc, b.acc), "two runs differ"
    assert torch.equal(a.acc, v.acc), "the strided views and their dense copy differ"
    assert bool((a.acc[0, ..., :2] > 0).all()) and bool((a.acc[1] == 0).all()) and a.count.tolist() == [3.0, 0.0]
    two = fresh()
    two.update(0, fd[:2], td[:2])
    two.update(0, fd[2:], td[2:])
    assert torch.equal(two.acc, a.acc) and torch.equal(two.count, a.count)
    acc64, _ = _acc64([(0, f, t)], a, 2)
    assert SO.error(two.acc[0].cpu().numpy(), acc64[0]) <= FWD
    # a channel alone == the same channel among others; channels= == the slice of the full result
    from paradis_model_amd.spectrum import Spectra
    lat, w = SO.cos_weights(H)
    alone = Spectra(["c1"], lat, 2, bands=BANDS3, weights=torch.from_numpy(w))
    alone.update(0, fd[:, 1:2].contiguous(), td[:, 1:2].contiguous())
    assert torch.equal(alone.acc[:, 0], a.acc[:, 1])
    sub = fresh(channels=["c2", "c0"])
    sub.update(0, fv, tv)
    assert sub.acc.shape[1] == 2 and torch.equal(sub.acc, a.acc[:, [2, 0]]) and sub.result()["names"] == ["c2", "c0"]
    # B == 0 leaves the accumulators untouched
    keep = two.acc.clone()
    two.update(0, fd[:0], td[:0])
    two.update(1, fd[:0], td[:0])
    assert torch.equal(two.acc, keep) and two.count.tolist() == [3.0, 0.0]
    two.reset()
    assert bool((two.acc == 0).all()) and np.isnan(two.result()["ratio"]).all()
    two.update(0, fd, td)
    assert torch.equal(two.acc, a.acc)                                  # and it counts again from zero


# ================================================================================================ 3. weights
def test_rows_of_weight_zero_are_left_out():
    """NaN in a row outside a band leaves that band finite and equal, bit for bit, to the run without the NaN; NaN in a
    row of weight zero in every band changes nothing; NaN inside a band propagates into that band and channel only
    (into all three sums: forecast and truth rows share one transform)"""
    rows = _consts()[0]
    B, C, H, W = 2, 2, rows + 1, 30
    f, t = SO.design(800, B, C, H, W)
    sp0 = _spectra(C, H, 1, 3)
    wb = sp0.band_w                                     # south | tropics | north-mid; rows poleward of 60 N: no weight
    nowhere = int(np.nonzero(wb.sum(0) == 0)[0][-1])
    south_only = int(np.nonzero((wb[0] > 0) & (wb[1] == 0))[0][0])
    sp0.update(0, f.cuda(), t.cuda())
    base = sp0.acc.clone()
    assert bool(torch.isfinite(base).all())

    def run(ff, tt):
        sp = _spectra(C, H, 1, 3)
        sp.update(0, ff.cuda(), tt.cuda())
        return sp.acc

    fn, tn = f.clone(), t.clone()
    fn[1, 0, nowhere, 3] = float("nan")
    tn[0, 1, nowhere, 0] = float("inf")                 # (the pivot cell of a row that is not read)
    assert torch.equal(run(fn, tn), base)
    fn, tn = f.clone(), t.clone()
    fn[0, 1, south_only, 7] = float("nan")
    got = run(fn, tn)
    assert torch.equal(got[:, :, 1:], base[:, :, 1:]) and torch.equal(got[:, 0], base[:, 0])
    assert bool(torch.isnan(got[0, 1, 0]).all())


# ================================================================================================ 4. the scorecard
@pytest.mark.parametrize("W", [30, 64])
def test_error_power_sums_to_the_scorecards_squared_rmse(W):
    """with the band weights equal to the scorecard's latitude weights, sum_k error_power is rmse^2 (Parseval for
    f - t); the bound is that of the scorecard's own test, 1e-5 of the largest value"""
    from paradis_model_amd.spectrum import Spectra
    from paradis_model_amd.verify import Scorecard
    rows = _consts()[0]
    B, C, H = 3, 3, rows + 1
    f, t = SO.design(900 + W, B, C, H, W)
    lat, w = SO.cos_weights(H)
    w32 = torch.from_numpy((w / w.mean()).astype(np.float32))
    card = Scorecard(_names(C), w32, 1)
    sp = Spectra(_names(C), lat, 1, weights=Scorecard.lat_weights_from(type("L", (), {"lat_weights_buf": w32})()))
    fd, td = f.cuda(), t.cuda()
    card.update(0, fd, td)
    sp.update(0, fd, td)
    rmse2 = card.result()["rmse"][0] ** 2
    total = sp.result()["error_power"][0, :, 0].sum(-1)
    e = float(np.abs(total - rmse2).max() / np.abs(rmse2).max())
    rel = float((np.abs(total - rmse2) / rmse2).max())
    print(f"SPECTRUM | W {W} | sum_k error_power against rmse^2 | e {e:.2e} | worst relative {rel:.2e}")
    assert e <= FWD
    d64 = (f.double() - t.double()) ** 2
    ref = (d64.mean(-1) * torch.from_numpy(w).view(1, 1, H)).sum(-1).mean(0).numpy() / w.sum()
    assert float((np.abs(total - ref) / ref).max()) <= FWD


# ================================================================================================ 5. the forecaster hook
@pytest.mark.parametrize("truth_normalized,graph,with_card", [(False, False, False), (True, True, True)])
def test_forecaster_hook(truth_normalized, graph, with_card):
    """run(spectra=..., truth=...) analyses the chunks it hands to on_chunk: bit for bit the accumulators of spectra
    updated by hand with those chunks; the chunks are those of a run without spectra; beside a scorecard both get the
    same states"""
    from paradis_model_amd.forecast import Forecaster, postprocess
    from paradis_model_amd.spectrum import Spectra
    from paradis_model_amd.verify import Scorecard
    from tests import forecast_oracle as FO
    from tests.test_hip_verify import _Collect, _rollout_setup, lat_weights
    model, spec, lat, lon, inputs, (H, W, B, S) = _rollout_setup()
    C = spec.num_channels
    norm = FO.normalised_state(31, spec.names, B, S, C, H, W).cuda()
    phys = torch.empty(B, S, C, H, W, device="cuda")
    for s in range(S):
        postprocess(norm[:, s], spec, lat, lon, phys, s)
    chosen = [spec.names[i] for i in (5, 0, C - 1)]
    bands = {"sh": (-90.0, 0.0), "nh": (0.0, 90.0)}

    def fresh():
        return Spectra(spec.names, lat, S, bands=bands, channels=chosen)

    fc = Forecaster(model, spec, lat, lon, output_frequency=1, write_every_n=2, graph=graph)
    plain = _Collect()
    fc.run(*inputs, plain)
    sp = fresh()
    card = Scorecard(spec.names, lat_weights(H), S) if with_card else None
    scored = _Collect()
    fc.run(*inputs, scored, spectra=sp, scorecard=card, truth=norm if truth_normalized else phys,
           truth_normalized=truth_normalized)
    assert [c[0] for c in scored.chunks] == [0, 2] and [c[1].shape[1] for c in scored.chunks] == [2, 1]
    for (s0, x), (s1, y) in zip(plain.chunks, scored.chunks):
        assert s0 == s1 and torch.equal(x, y)                               # the chunk contents are unchanged
    states = torch.cat([c[1] for c in scored.chunks], dim=1)
    by_hand = fresh()
    for s in range(S):
        by_hand.update(s, states[:, s].cuda(), phys[:, s])
    assert torch.equal(sp.acc, by_hand.acc) and torch.equal(sp.count, by_hand.count)
    assert sp.count.tolist() == [float(B)] * S and bool(torch.isfinite(sp.acc).all())
    if with_card:
        alone = Scorecard(spec.names, lat_weights(H), S)
        fc.run(*inputs, None, scorecard=alone, truth=norm if truth_normalized else phys,
               truth_normalized=truth_normalized)
        assert torch.equal(card.acc, alone.acc)
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, spectra=sp, truth=phys[:, :2])                # a wrong n_stored: before the rollout
    with pytest.raises(ValueError, match="truth"):
        fc.run(*inputs, None, spectra=sp)
    with pytest.raises(ValueError, match="leads"):
        fc.run(*inputs, None, spectra=Spectra(spec.names, lat, S - 1), truth=phys)
    assert torch.equal(sp.acc, by_hand.acc)
