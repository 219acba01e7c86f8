"""CPU: zonal power spectra without a device - the fp64 oracle (tests/spectrum_oracle.py) against closed forms, the
error of its two float32 yardsticks on every input design, bands as weight rows, the host side of ``spectrum.Spectra``
(argument errors, ``result`` / ``effective_resolution`` arithmetic, ``table``) and of ``Forecaster.run(spectra=...)``,
and the C-ABI symbols of ``csrc/spectrum.hip`` with their argument rejection before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import spectrum_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("paradis_spectrum_rows", "paradis_spectrum_fft_max_w", "paradis_spectrum_direct_max_w",
           "paradis_spectrum_schedule", "paradis_spectrum_ws_bytes", "paradis_spectrum_update")
FWD = 1e-5                      # the project's forward ceiling
NAMES = ["t2m", "z500", "q850"]
LAT = np.array([-60.0, -30.0, 0.0, 30.0, 60.0])


# ================================================================================================ 1. the oracle
@pytest.mark.parametrize("W,k,a", [(8, 1, 1.5), (8, 3, 0.25), (30, 7, 2.0), (64, 31, 1.0)])
def test_oracle_single_cosine(W, k, a):
    i = np.arange(W)
    x = a * np.cos(2 * np.pi * k * i / W + 0.3)
    p = SO.row_spectra(x, x)
    want = np.zeros(W // 2 + 1)
    want[k] = a * a / 2
    assert np.allclose(p[:, 0], want, rtol=0, atol=1e-14 * a * a) and np.array_equal(p[:, 0], p[:, 1])
    assert np.allclose(p[:, 2], want, rtol=0, atol=1e-14 * a * a)


@pytest.mark.parametrize("W", [4, 8, 30])
def test_oracle_nyquist_and_mean(W):
    i = np.arange(W)
    a, m = 0.75, -3.0
    x = m + a * np.cos(np.pi * i)                       # k = K: the full a^2, not a^2 / 2
    p = SO.row_spectra(x, x)[:, 0]
    want = np.zeros(W // 2 + 1)
    want[0], want[-1] = m * m, a * a
    assert np.allclose(p, want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("W", [4, 6, 14, 50, 1440])
def test_oracle_parseval(W):
    f, t = SO.design(7, 2, 2, 3, W)
    p = SO.row_spectra(f, t)
    f64, t64 = f.double().numpy(), t.double().numpy()
    assert np.allclose(p[..., 0].sum(-1), (f64 ** 2).mean(-1), rtol=1e-12)
    assert np.allclose(p[..., 1].sum(-1), (t64 ** 2).mean(-1), rtol=1e-12)
    assert np.allclose(p[..., 2].sum(-1), (f64 * t64).mean(-1), rtol=1e-12)
    # error_power is the spectrum of f - t: its sum over k is the mean squared error of the row
    err = p[..., 0] + p[..., 1] - 2 * p[..., 2]
    assert np.allclose(err.sum(-1), ((f64 - t64) ** 2).mean(-1), rtol=1e-9)


@pytest.mark.parametrize("phi", [0.0, 0.4, np.pi / 2, 2.5, np.pi])
def test_oracle_phase_shift_gives_cos_phi_coherence(phi):
    W, k = 30, 4
    i = np.arange(W)
    f = 1.3 * np.cos(2 * np.pi * k * i / W)[None, None, None, :]
    t = 0.7 * np.cos(2 * np.pi * k * i / W + phi)[None, None, None, :]
    r = SO.report(*SO.accumulate([(0, f, t)], np.ones((1, 1)), 1))
    assert abs(r["coherence"][0, 0, 0, k] - np.cos(phi)) <= 1e-13
    assert abs(r["ratio"][0, 0, 0, k] - (1.3 / 0.7) ** 2) <= 1e-12


def test_oracle_leads_counts_and_zero_weight_rows():
    f, t = SO.design(11, 3, 2, 4, 8)
    wb = np.array([[1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 5.0]])
    acc, n = SO.accumulate([(1, f[:2], t[:2]), (1, f[2:], t[2:])], wb, 3)
    whole, n2 = SO.accumulate([(1, f, t)], wb, 3)
    assert np.array_equal(acc, whole) and n.tolist() == [0.0, 3.0, 0.0] and n2.tolist() == n.tolist()
    r = SO.report(acc, n)
    assert all(np.isnan(r[q][0]).all() and np.isnan(r[q][2]).all() and np.isfinite(r[q][1]).all() for q in SO.QUANTITIES)
    # a NaN in a row of weight 0 does not reach the band; band 1 is the plain spectrum of row 3
    fn = f.clone()
    fn[:, :, 2, 3] = float("nan")
    assert np.array_equal(SO.band_spectra(fn, t, wb), SO.band_spectra(f, t, wb))
    assert np.allclose(SO.band_spectra(f, t, wb)[:, :, 1], SO.row_spectra(f, t)[:, :, 3], rtol=1e-15)
    fn[:, :, 3, 0] = float("nan")
    S = SO.band_spectra(fn, t, wb)
    assert np.isfinite(S[:, :, 0]).all() and np.isnan(S[:, :, 1, :, 0]).all()


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("W", [4, 8, 14, 30, 64, 254, 1440])
def test_yardsticks_stay_under_a_third_of_the_ceiling(W, offset):
    """The inputs of tests/test_hip_spectrum.py: both float32 CPU evaluations (FFT and matrix DFT, same pivot) are
    within a third of the forward ceiling of the fp64 oracle, so the GPU bound max(3 e_cpu, 1e-6) never exceeds it;
    without the pivot the offset design is beyond that GPU bound."""
    H = 3
    f, t = SO.design(40 + W, 2, 2, H, W, offset)
    _, w = SO.cos_weights(H)
    wb = w[None]
    if not offset:
        SO.check_design(f, t, wb)
    S64 = SO.band_spectra(f, t, wb).sum(0)
    es = [SO.error(SO.band_spectra(f, t, wb, m).sum(0), S64) for m in ("fft32", "dft32")]
    print(f"SPECTRUM | W {W} offset {offset} | e_fft32 {es[0]:.2e} | e_dft32 {es[1]:.2e}")
    assert max(es) <= FWD / 3, es
    if offset:
        e_np = SO.error(SO.band_spectra(f, t, wb, "fft32", pivot=False).sum(0), S64)
        print(f"SPECTRUM | W {W} without the pivot {e_np:.2e}")
        assert e_np > max(3 * max(es), 1e-6), e_np


# ================================================================================================ 2. bands
def test_bands_become_weight_rows():
    from paradis_model_amd.spectrum import Spectra, band_weights
    w = np.array([1.0, 2.0, 3.0, 2.0, 1.0])
    wb = band_weights(LAT, w, {"south": (-90, -30), "tropics": (-30, 30), "all": (-90, 90)})
    assert wb.dtype == np.float64 and wb.tolist() == [[1, 2, 0, 0, 0], [0, 2, 3, 2, 0], [1, 2, 3, 2, 1]]
    assert band_weights(LAT, w, {"edge": (30.0, 30.0)}).tolist() == [[0, 0, 0, 2, 0]]      # a row exactly on both edges
    for bad in ({"empty": (31, 59)}, {"gone": (61, 90)}, {"rev": (30, -30)}, {"nan": (float("nan"), 10)}, {"one": (3,)},
                {"zero-weight": (0, 0)}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            band_weights(LAT, np.array([1.0, 2.0, 0.0, 2.0, 1.0]), bad)
    s = Spectra(NAMES, LAT, 2, device="cpu")
    assert s.bands == ["global"] and np.allclose(s.band_w, np.cos(np.deg2rad(LAT))[None], rtol=1e-15)
    poles = Spectra(NAMES, [-90.0, 0.0, 90.0], 1, device="cpu")
    assert poles.band_w.tolist() == [[0.0, 1.0, 0.0]]                       # cos(90 deg) is 0, not 6e-17
    s = Spectra(NAMES, LAT, 2, bands={"nh": (0, 90), "sh": (-90, 0)}, weights=torch.tensor(w).float().view(1, 1, 5, 1),
                channels=["q850", "t2m"], device="cpu")
    assert s.bands == ["nh", "sh"] and s.band_w.tolist() == [[0, 0, 3, 2, 1], [1, 2, 3, 0, 0]]
    assert s.names == ["q850", "t2m"] and s.index == [2, 0] and s.all_names == NAMES
    loss = type("L", (), {"lat_weights_buf": torch.tensor(w).view(1, 1, -1, 1)})()
    assert Spectra.lat_weights_from(loss) is loss.lat_weights_buf
    assert Spectra(NAMES, LAT, 1, weights=Spectra.lat_weights_from(loss), device="cpu").band_w.tolist() == [w.tolist()]


# ================================================================================================ 3. host logic
def test_spectra_constructor_errors():
    from paradis_model_amd.spectrum import Spectra
    with pytest.raises(ValueError, match="names"):
        Spectra([], LAT, 3, device="cpu")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_leads"):
            Spectra(NAMES, LAT, bad, device="cpu")
    for bad in ([], [0.0, 91.0], [0.0, float("nan")]):
        with pytest.raises(ValueError, match="lat_deg"):
            Spectra(NAMES, bad, 3, device="cpu")
    for bad in (torch.zeros(5), torch.tensor([1.0, -1.0, 1.0, 1.0, 1.0]), torch.ones(4), torch.ones(5, dtype=torch.int32),
                torch.tensor([1.0, float("inf"), 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match="weights"):
            Spectra(NAMES, LAT, 3, weights=bad, device="cpu")
    for bad in ({}, [(-90, 90)]):
        with pytest.raises(ValueError, match="bands"):
            Spectra(NAMES, LAT, 3, bands=bad, device="cpu")
    with pytest.raises(ValueError, match="polar"):
        Spectra(NAMES, LAT, 3, bands={"polar": (70, 90)}, device="cpu")
    with pytest.raises(ValueError, match="nope"):
        Spectra(NAMES, LAT, 3, channels=["t2m", "nope"], device="cpu")
    with pytest.raises(ValueError, match="repeat"):
        Spectra(NAMES, LAT, 3, channels=["t2m", "t2m"], device="cpu")
    with pytest.raises(ValueError, match="channels"):
        Spectra(NAMES, LAT, 3, channels=[], device="cpu")
    s = Spectra(NAMES, LAT, 3, device="cpu")
    assert s.acc is None and s.count.shape == (3,) and s.count.dtype == torch.float64
    with pytest.raises(RuntimeError, match="no update"):
        s.result()
    for bad in (7, 0, 8192, 6.5, 2 * 127 + 2 * 2):
        with pytest.raises(ValueError, match="longitudes"):
            s.bind(bad)
    s.bind(8)
    assert s.acc.shape == (3, 3, 1, 5, 3) and s.acc.dtype == torch.float64 and s.W == 8
    s.bind(8)
    with pytest.raises(ValueError, match="bound"):
        s.bind(16)


def test_spectra_update_argument_errors_on_cpu_tensors():
    from paradis_model_amd.spectrum import Spectra
    H, W = 5, 8
    f = torch.zeros(2, 3, H, W)
    s = Spectra(NAMES, LAT, 3, device="cpu")
    for lead in (-1, 3, 1.0, None, True):
        with pytest.raises(ValueError, match="lead"):
            s.update(lead, f, f)
    with pytest.raises(ValueError, match="forecast"):
        s.update(0, f.double(), f)
    with pytest.raises(ValueError, match="truth"):
        s.update(0, f, f.double())
    with pytest.raises(ValueError, match="forecast"):
        s.update(0, torch.zeros(2, 4, H, W), torch.zeros(2, 4, H, W))
    with pytest.raises(ValueError, match="forecast"):
        s.update(0, f[0], f[0])
    with pytest.raises(ValueError, match="truth"):
        s.update(0, f, torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="forecast"):
        s.update(0, torch.zeros(2, 3, H, 2 * W)[..., ::2], f)
    with pytest.raises(ValueError, match="truth"):
        s.update(0, f, torch.zeros(2, 3, W, H).transpose(-1, -2))
    for bad_w in (7, 22 * 13, 8192):                      # odd; not smooth and past the direct limit; past the fft limit
        x = torch.zeros(1, 3, H, bad_w)
        with pytest.raises(ValueError, match="longitudes"):
            s.update(0, x, x)
    with pytest.raises(RuntimeError, match="MI355X"):        # valid arguments on the CPU: there is no CPU fallback
        s.update(0, f, f)
    assert s.acc is None and (s.count == 0).all()
    s.bind(16)
    with pytest.raises(ValueError, match="longitudes"):
        s.update(0, f, f)                                    # another W than the one the accumulators are bound to


def _filled():
    from paradis_model_amd.spectrum import Spectra
    s = Spectra(NAMES, LAT, 3, bands={"nh": (0, 90), "sh": (-90, 0)}, channels=["z500", "t2m"], device="cpu")
    s.bind(8)
    #                     ff    tt   ft        k = 0 .. 4
    s.acc[0, 0, 0] = torch.tensor([[8.0, 8.0, 8.0], [4.0, 16.0, 4.0], [2.0, 8.0, 0.0], [1.0, 4.0, -2.0], [0.0, 2.0, 0.0]],
                                  dtype=torch.float64)
    s.acc[0, 0, 1] = s.acc[0, 0, 0] * 3.0
    s.acc[0, 1, 0] = torch.tensor([[2.0, 2.0, 2.0], [4.0, 4.0, 4.0], [6.0, 8.0, 6.0], [2.0, 2.0, 2.0], [1.0, 4.0, 2.0]],
                                  dtype=torch.float64)
    s.acc[0, 1, 1] = 1.0
    s.acc[2] = s.acc[0] * 2.0
    s.count[0], s.count[2] = 2.0, 4.0
    return s


def test_spectra_result_arithmetic_from_a_hand_filled_accumulator():
    from paradis_model_amd.spectrum import QUANTITIES, Spectra
    s = _filled()
    r = s.result()
    assert r["names"] == ["z500", "t2m"] and r["bands"] == ["nh", "sh"] and r["count"].tolist() == [2.0, 0.0, 4.0]
    assert r["wavenumber"].tolist() == [0, 1, 2, 3, 4]
    for q in QUANTITIES:
        assert r[q].shape == (3, 2, 2, 5) and r[q].dtype == np.float64
        assert np.isnan(r[q][1]).all(), q                                       # the lead never updated
    assert r["power_forecast"][0, 0, 0].tolist() == [4.0, 2.0, 1.0, 0.5, 0.0]
    assert r["power_truth"][0, 0, 0].tolist() == [4.0, 8.0, 4.0, 2.0, 1.0]
    assert r["cospectrum"][0, 0, 0].tolist() == [4.0, 2.0, 0.0, -1.0, 0.0]
    assert r["ratio"][0, 0, 0].tolist() == [1.0, 0.25, 0.25, 0.25, 0.0]
    assert r["coherence"][0, 0, 0, :4].tolist() == [1.0, 0.5, 0.0, -1.0] and np.isnan(r["coherence"][0, 0, 0, 4])
    assert r["error_power"][0, 0, 0].tolist() == [0.0, 6.0, 5.0, 4.5, 1.0]
    assert np.array_equal(r["ratio"][2], r["ratio"][0], equal_nan=True)         # twice the sums over twice the count
    assert np.array_equal(r["power_truth"][2], r["power_truth"][0])
    want = SO.report(s.acc.numpy(), s.count.numpy())
    for q in QUANTITIES + ("count", "wavenumber"):
        assert np.array_equal(r[q], want[q], equal_nan=True), q
    r2 = s.result(sync_dist=True)                                               # no process group: a plain read
    assert all(np.array_equal(r2[q], r[q], equal_nan=True) for q in QUANTITIES)
    # effective resolution: first k >= 1 with ratio < threshold, K + 1 if none; NaN is not below anything
    eff = Spectra.effective_resolution(r)
    assert eff.shape == (3, 2, 2) and eff.dtype == np.int64
    assert eff[0].tolist() == [[1, 1], [4, 5]] and eff[1].tolist() == [[5, 5], [5, 5]]
    assert Spectra.effective_resolution(r, threshold=0.2)[0].tolist() == [[4, 4], [5, 5]]
    assert Spectra.effective_resolution(r, threshold=0.8)[0].tolist() == [[1, 1], [2, 5]]
    for thr in (0.2, 0.5, 0.8, 2.0):
        assert np.array_equal(Spectra.effective_resolution(r, thr), SO.effective_resolution(r["ratio"], thr))
    s.reset()
    assert (s.acc == 0).all() and (s.count == 0).all() and np.isnan(s.result()["ratio"]).all()


def test_spectra_result_sync_dist_makes_one_all_reduce(tmp_path, monkeypatch):
    import torch.distributed as dist
    s = _filled()
    want = s.result()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        calls = []
        real = dist.all_reduce
        monkeypatch.setattr(dist, "all_reduce", lambda t, **kw: (calls.append(tuple(t.shape)), real(t, **kw))[1])
        keep = s.acc.clone()
        got = s.result(sync_dist=True)
        assert calls == [(s.acc.numel() + 3,)] and torch.equal(s.acc, keep)
        assert s.result() is not None and len(calls) == 1
    finally:
        dist.destroy_process_group()
    for q in SO.QUANTITIES + ("count",):
        assert np.array_equal(got[q], want[q], equal_nan=True), q


def test_spectra_table_formatting():
    from paradis_model_amd.spectrum import Spectra
    r = _filled().result()
    text = Spectra.table(r, "z500")
    lines = text.split("\n")
    assert lines[0] == "z500 / nh"
    blocks = "\n".join(lines[1:]).split("\n\n")
    assert [b.split()[0] for b in blocks] == ["power_truth", "ratio", "coherence"]
    assert lines[1].split() == ["power_truth", "count", "k=1", "k=2", "k=4"]
    assert lines[2].split() == ["0", "2", "8.0000e+00", "4.0000e+00", "1.0000e+00"]
    assert lines[3].split() == ["1", "0", "nan", "nan", "nan"]
    assert all(len(b.split("\n")) == 4 for b in blocks)
    assert len({len(line) for line in blocks[0].split("\n")}) == 1               # aligned columns
    sub = Spectra.table(r, "t2m", band="sh", wavenumbers=[0, 3])
    assert sub.split("\n")[0] == "t2m / sh" and sub.split("\n")[1].split() == ["power_truth", "count", "k=0", "k=3"]
    assert sub.split("\n")[2].split() == ["0", "2", "5.0000e-01", "5.0000e-01"]
    for kw, word in ((dict(channel="q850"), "q850"), (dict(channel="t2m", band="tropics"), "tropics"),
                     (dict(channel="t2m", wavenumbers=[5]), "wavenumber")):
        with pytest.raises(ValueError, match=word):
            Spectra.table(r, **kw)


# ================================================================================================ 4. the forecaster hook
def test_forecaster_run_refusals_with_spectra():
    from paradis_model_amd.forecast import Forecaster, PostSpec
    from paradis_model_amd.spectrum import Spectra
    H, W = 5, 8
    spec = PostSpec.from_features(NAMES, [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    fc = Forecaster(None, spec, LAT, np.zeros(W), graph=False)
    inp, forc, const = torch.zeros(1, 1, 6, H, W), torch.zeros(1, 2, H, W, 1), torch.zeros(1, 1, H, W, 1)
    with pytest.raises(ValueError, match="truth"):
        fc.run(inp, forc, const, None, spectra=Spectra(NAMES, LAT, 2, device="cpu"), truth=None)
    # the checks that follow the device check of the inputs, on the method that makes them
    good = torch.zeros(1, 2, 3, H, W)
    args = (None, good, False, None, 1, 2, 3, H, W)
    with pytest.raises(ValueError, match="truth"):
        fc._check_verification(None, good[:, :1], False, None, 1, 2, 3, H, W, Spectra(NAMES, LAT, 2, device="cpu"))
    with pytest.raises(ValueError, match="leads"):
        fc._check_verification(*args, Spectra(NAMES, LAT, 1, device="cpu"))
    with pytest.raises(ValueError, match="names"):
        fc._check_verification(*args, Spectra(NAMES[::-1], LAT, 2, device="cpu"))
    with pytest.raises(ValueError, match="clim_index"):
        fc._check_verification(None, good, False, torch.zeros(1, 2, dtype=torch.int32), 1, 2, 3, H, W,
                               Spectra(NAMES, LAT, 2, device="cpu"))
    with pytest.raises(ValueError, match="scorecard"):                  # as before: truth alone goes with nothing
        fc._check_verification(None, good, False, None, 1, 2, 3, H, W)
    with pytest.raises(RuntimeError, match="MI355X"):                   # every host check passed: the device check
        fc._check_verification(*args, Spectra(NAMES, LAT, 2, channels=["z500"], device="cpu"))


# ================================================================================================ 5. the C ABI
def test_spectrum_symbols_are_declared_exported_and_bound():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    sig = _lib.SIGNATURES["paradis_spectrum_update"][1]
    assert len(sig) == 18 and sig[1] is ctypes.c_int64 and sig[3] is ctypes.c_int64 and sig[5] is ctypes.c_int
    assert _lib.SIGNATURES["paradis_spectrum_ws_bytes"][0] is ctypes.c_size_t
    assert _lib.lib.paradis_abi_version() == 10
    L = _lib.lib
    assert L.paradis_spectrum_rows() >= 1 and L.paradis_spectrum_fft_max_w() >= 1440
    dmax = L.paradis_spectrum_direct_max_w()
    assert dmax >= 26 and dmax % 2 == 0 and L.paradis_spectrum_schedule(dmax) == 2     # the limit itself is a direct W


def test_spectrum_schedule_choice():
    from paradis_model_amd import _lib, spectrum
    L = _lib.lib
    fmax, dmax = L.paradis_spectrum_fft_max_w(), L.paradis_spectrum_direct_max_w()
    for W in (64, 256, 1440, 30, 50, 4, 6, 8, 90, 2):
        assert L.paradis_spectrum_schedule(W) == 1 and spectrum.schedule(W) == "fft", W
    for W in (14, 22, 26, dmax):
        assert L.paradis_spectrum_schedule(W) == 2 and spectrum.schedule(W) == "direct", W
    for W in (7, 1, 0, -4, 15, 1441):
        assert L.paradis_spectrum_schedule(W) == 0 and spectrum.schedule(W) is None, W
    smooth_past = 2
    while smooth_past <= fmax:
        smooth_past *= 2
    assert L.paradis_spectrum_schedule(smooth_past) == 0                  # a smooth W past the fft limit
    rough_past = dmax + 2
    while L.paradis_spectrum_schedule(rough_past) == 1:                   # the next even W that is not smooth
        rough_past += 2
    assert L.paradis_spectrum_schedule(rough_past) == 0
    tw = spectrum.twiddle_table(12)
    assert tw.dtype == np.float32 and tw.shape == (12, 2)
    j = np.arange(12)
    assert np.array_equal(tw[:, 0], np.cos(2 * np.pi * j / 12).astype(np.float32))
    assert np.array_equal(tw[:, 1], (-np.sin(2 * np.pi * j / 12)).astype(np.float32))


def test_spectrum_workspace_holds_the_partials():
    """double [B*Cs][ceil(H / rows)][R][3][K + 1]"""
    from paradis_model_amd import _lib
    L = _lib.lib
    rows = L.paradis_spectrum_rows()
    for (B, Cs, H, W, R) in ((3, 2, 9, 30, 1), (1, 96, 721, 1440, 3), (2, 1, rows, 64, 2), (2, 1, rows + 1, 64, 2)):
        groups = -(-H // rows)
        assert L.paradis_spectrum_ws_bytes(B, Cs, H, W, R) >= B * Cs * groups * R * 3 * (W // 2 + 1) * 8
    assert L.paradis_spectrum_ws_bytes(0, 2, 9, 30, 1) == 0 and L.paradis_spectrum_ws_bytes(1, 2, 9, 30, 0) == 0


def test_spectrum_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first

    def call(fc=fake, truth=fake, chan=None, Cs=3, wb=fake, wsum=fake, tw=fake, acc=fake, count=fake, ws=fake, B=2, C=3,
             H=4, W=8, R=1, fc_bs=96, truth_bs=96):
        return L.paradis_spectrum_update(fc, fc_bs, truth, truth_bs, chan, Cs, wb, wsum, tw, acc, count, ws, B, C, H, W,
                                         R, None)

    dmax, fmax = L.paradis_spectrum_direct_max_w(), L.paradis_spectrum_fft_max_w()
    for W in (7, dmax + 2 if L.paradis_spectrum_schedule(dmax + 2) == 0 else dmax + 4, 2 * fmax):
        assert call(W=W, fc_bs=10 ** 6, truth_bs=10 ** 6) == 1 and "even" in _lib.last_error(), W
        assert call(W=W, B=0) == 1 and "even" in _lib.last_error(), W
    for R in (0, -1, 65):
        assert call(R=R) == 1 and "bands" in _lib.last_error(), R
    assert call(W=fmax, R=64, fc_bs=10 ** 6, truth_bs=10 ** 6) == 1 and "LDS" in _lib.last_error()   # 64 x 49 KB
    for kw in (dict(C=0), dict(H=0), dict(W=0), dict(Cs=0), dict(B=-1)):
        assert call(**kw) == 1 and "shape" in _lib.last_error(), kw
    assert call(Cs=2) == 1 and "channel table" in _lib.last_error()
    assert call(acc=None) == 1 and "acc" in _lib.last_error()
    assert call(count=None) == 1 and "count" in _lib.last_error()
    assert call(ws=None) == 1 and "ws" in _lib.last_error()
    for kw in (dict(fc=None), dict(truth=None), dict(wb=None), dict(wsum=None), dict(tw=None)):
        assert call(**kw) == 1 and "null" in _lib.last_error(), kw
    assert call(fc_bs=95) == 1 and "stride" in _lib.last_error()
    assert call(B=2 ** 24, Cs=2 ** 8, C=2 ** 8, fc_bs=2 ** 20, truth_bs=2 ** 20) == 1 and "grid" in _lib.last_error()
    # B == 0: nothing to do, whatever the pointers
    assert L.paradis_spectrum_update(None, 0, None, 0, None, 3, None, None, None, None, None, None, 0, 3, 4, 8, 1,
                                     None) == 0
