"""Zonal power spectra in plain numpy: a restatement of the conventions of ``paradis_model_amd/spectrum.py`` (the
project's own definition, in the spirit of WeatherBench-2's ``ZonalEnergySpectrum``, not pinned against it) that imports
nothing from the package.

Forecast ``f`` and truth ``t`` ``[B, C, H, W]``, ``W`` even, ``K = W / 2``; per row, through ``np.fft.rfft`` in float64::

    X[h,k] = rfft(x[h])[k] / W      m_k = 1 for k in {0, K}, else 2
    pf = m_k |F|^2     pt = m_k |T|^2     co = m_k Re(F conj T)

band weights ``wb [R, H] >= 0``: ``S[r,k] = sum_{h: wb[r,h] != 0} wb[r,h] p[h,k] / sum_h wb[r,h]``, accumulated over the
samples as ``acc [n_leads, Cs, R, K + 1, 3] = {sum S_ff, sum S_tt, sum S_ft}`` with ``count [n_leads]``, and reported as
``power_forecast``, ``power_truth``, ``cospectrum`` (sum / count), ``ratio = S_ff / S_tt``, ``coherence = S_ft /
sqrt(S_ff S_tt)``, ``error_power = S_ff + S_tt - 2 S_ft``.

``method="rfft"`` is the float64 reference.  The two float32 yardsticks of the GPU tests transform, as the kernel does,
ONE complex row ``z = (f - p) + i (t - p)`` with the pivot ``p = t[h, 0]`` in complex64 on the CPU - ``"fft32"``:
``torch.fft.fft``; ``"dft32"``: a complex64 matrix product with ``exp(-2 pi i j k / W)`` (built in float64, rounded
once) - and separate ``F = (Z_k + conj Z_{W-k}) / 2W``, ``T = (Z_k - conj Z_{W-k}) / 2iW`` in float64, ``k = 0``
restored as ``X_0 + p``; ``pivot=False`` leaves the pivot out (what the offset design is there to catch).

Input designs (``design``): every truth row has coefficients of amplitude ``k^-1.5`` with random phases (power ``k^-3``:
up to ten decades at W = 1440), spikes at k = 1, K - 1 and K, a mean of 2 .. 2.5 times the k = 1 amplitude, and every
plane a scale of its own (``10^u``, u in [-2, 3]).  The forecast is the truth through the transfer function ``g(k) =
0.65 / sqrt(1 + (3 k / K)^2)`` plus noise of amplitude ``0.3 |c_k|`` whose phase lies 60 .. 120 degrees off the truth's
(either side): per row and k >= 1, ``ratio = (g + 0.3 cos a)^2 + 0.09 sin^2 a`` lies in (0.01, 0.73) and ``coherence =
(g + 0.3 cos a) / sqrt(ratio)`` in (0.17, 0.96), so both stay strictly inside (0, 1) after any weighted mean (Cauchy-
Schwarz); at k = K both coefficients are real, so a single row's coherence there is 1.  ``offset=True`` adds 1e5 to
both fields - what 500 hPa geopotential looks like - with plane scales ``10^u``, u in [0, 2]: float32 at 1e5 resolves
0.008, which white-noises the small scales of the stored fields, so ``check_design`` is for the plain variant.
"""
import numpy as np
import torch

QUANTITIES = ("power_forecast", "power_truth", "cospectrum", "ratio", "coherence", "error_power")
OFFSET = 1.0e5


# ================================================================================================ the transform
def _mult(W):
    m = np.full(W // 2 + 1, 2.0)
    m[0] = m[-1] = 1.0
    return m


def _coefficients(f, t, method, pivot):
    """(F, T) complex128 ``[..., K + 1]`` of float rows ``f``, ``t`` ``[..., W]`` (numpy; float32 for the yardsticks)"""
    W = f.shape[-1]
    K = W // 2
    if method == "rfft":
        return np.fft.rfft(f.astype(np.float64), axis=-1) / W, np.fft.rfft(t.astype(np.float64), axis=-1) / W
    f32, t32 = f.astype(np.float32), t.astype(np.float32)
    p = t32[..., :1] if pivot else np.zeros_like(t32[..., :1])
    z = torch.complex(torch.from_numpy(np.ascontiguousarray(f32 - p)), torch.from_numpy(np.ascontiguousarray(t32 - p)))
    assert z.dtype == torch.complex64
    if method == "fft32":
        Z = torch.fft.fft(z, dim=-1)
    elif method == "dft32":
        jk = np.outer(np.arange(W), np.arange(W)) % W
        M = torch.from_numpy(np.exp(-2j * np.pi * jk / W).astype(np.complex64))
        Z = z.reshape(-1, W) @ M
        Z = Z.reshape(z.shape)
    else:
        raise ValueError(method)
    assert Z.dtype == torch.complex64
    Z = Z.numpy().astype(np.complex128)
    k = np.arange(K + 1)
    Zk, Zc = Z[..., k], np.conj(Z[..., (W - k) % W])
    F, T = (Zk + Zc) / (2.0 * W), (Zk - Zc) / (2.0j * W)
    F[..., 0] += p[..., 0].astype(np.float64)
    T[..., 0] += p[..., 0].astype(np.float64)
    return F, T


def row_spectra(f, t, method="rfft", pivot=True):
    """float64 ``[..., K + 1, 3]``: (pf, pt, co) of every row"""
    f = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert f.shape == t.shape and f.shape[-1] % 2 == 0
    F, T = _coefficients(f, t, method, pivot)
    m = _mult(f.shape[-1])
    return np.stack([m * np.abs(F) ** 2, m * np.abs(T) ** 2, m * (F * np.conj(T)).real], axis=-1)


def band_spectra(f, t, wb, method="rfft", pivot=True):
    """float64 ``[B, C, R, K + 1, 3]``: S_ff, S_tt, S_ft of every sample, channel and band; rows of weight 0 are left
    out of their band, not multiplied in"""
    p = row_spectra(f, t, method, pivot)                       # [B, C, H, K + 1, 3]
    wb = np.asarray(wb, np.float64)
    out = np.zeros(p.shape[:2] + (wb.shape[0],) + p.shape[3:])
    for r in range(wb.shape[0]):
        use = np.nonzero(wb[r])[0]
        assert use.size > 0 and (wb[r] >= 0).all()
        out[:, :, r] = np.einsum("h,bchkf->bckf", wb[r, use], p[:, :, use]) / wb[r].sum()
    return out


def accumulate(updates, wb, n_leads, channels=None, method="rfft", pivot=True):
    """``updates``: a list of ``(lead, f, t)`` -> ``(acc [n_leads, Cs, R, K + 1, 3], count [n_leads])``"""
    acc, count = None, np.zeros(n_leads)
    for lead, f, t in updates:
        if channels is not None:
            f, t = f[:, channels], t[:, channels]
        S = band_spectra(f, t, wb, method, pivot)
        if acc is None:
            acc = np.zeros((n_leads,) + S.shape[1:])
        for b in range(S.shape[0]):
            acc[lead] += S[b]
        count[lead] += S.shape[0]
    return acc, count


def report(acc, count):
    """the reported values of ``Spectra.result``: NaN where a lead was never updated"""
    acc, count = np.asarray(acc, np.float64), np.asarray(count, np.float64)
    n = count.reshape(-1, 1, 1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ff, tt, ft = acc[..., 0] / n, acc[..., 1] / n, acc[..., 2] / n
        res = {"power_forecast": ff, "power_truth": tt, "cospectrum": ft, "ratio": ff / tt,
               "coherence": ft / np.sqrt(ff * tt), "error_power": ff + tt - 2.0 * ft}
    for q in QUANTITIES:
        res[q] = np.where(n > 0, res[q], np.nan)
    res["wavenumber"] = np.arange(acc.shape[3])
    res["count"] = count.copy()
    return res


def effective_resolution(ratio, threshold=0.5):
    """first k >= 1 with ratio < threshold, K + 1 if none; by a plain loop"""
    ratio = np.asarray(ratio)
    out = np.full(ratio.shape[:-1], ratio.shape[-1], np.int64)
    for idx in np.ndindex(*ratio.shape[:-1]):
        for k in range(1, ratio.shape[-1]):
            if ratio[idx + (k,)] < threshold:
                out[idx] = k
                break
    return out


# ================================================================================================ the error norm
def error(S, S64):
    """the norm of the spectrum tests, over accumulated sums ``[Cs, R, K + 1, 3]`` of one lead: the largest over
    (channel, band) of
      k >= 1:  max_k,field |S - S64| / sqrt(max(S64_ff[k], S64_tt[k]) * max(tot_ff, tot_tt)),  tot = sum_{k >= 1} S64
      k == 0:  the relative error of S_ff and S_tt"""
    S, S64 = np.asarray(S, np.float64), np.asarray(S64, np.float64)
    worst = 0.0
    for c in range(S64.shape[0]):
        for r in range(S64.shape[1]):
            a, b = S[c, r], S64[c, r]
            if not np.isfinite(a).all():
                return float("inf")
            e0 = max(abs(a[0, 0] - b[0, 0]) / abs(b[0, 0]), abs(a[0, 1] - b[0, 1]) / abs(b[0, 1]))
            tot = max(b[1:, 0].sum(), b[1:, 1].sum())
            scale = np.sqrt(np.maximum(b[1:, 0], b[1:, 1]) * tot)
            ek = (np.abs(a[1:] - b[1:]).max(axis=-1) / scale).max()
            worst = max(worst, float(e0), float(ek))
    return worst


# ================================================================================================ inputs
def design(seed, B, C, H, W, offset=False):
    """(forecast, truth) float32 torch ``[B, C, H, W]`` on the CPU, by the module docstring"""
    rng = np.random.default_rng(seed)
    K = W // 2
    k = np.arange(K + 1, dtype=np.float64)
    amp = np.zeros(K + 1)
    amp[1:] = k[1:] ** -1.5
    amp[1] += 1.0                                              # the spikes (they add up where K - 1 or K is 1)
    amp[K - 1] += 0.3 if K > 1 else 0.0
    amp[K] += 0.2
    shape = (B, C, H, K + 1)
    c = amp * np.exp(2j * np.pi * rng.random(shape))
    g = 0.65 / np.sqrt(1.0 + (3.0 * k / K) ** 2)
    ang = (np.pi / 3.0) * (1.0 + rng.random(shape)) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    d = c * (g + 0.3 * np.exp(1j * ang))
    mean = 2.0 + 0.5 * rng.random(shape[:-1])
    c[..., 0] = mean                                           # the row means: forecast 3 % .. 8 % off
    d[..., 0] = mean * (1.03 + 0.05 * rng.random(shape[:-1]))
    c[..., K] = c[..., K].real + np.sign(c[..., K].real) * 0.05 * amp[K]          # the Nyquist coefficient is real
    d[..., K] = c[..., K] * (g[K] + 0.3 * np.cos(ang[..., K]))
    u = rng.random((B, C, 1, 1))
    scale = 10.0 ** (2.0 * u if offset else -2.0 + 5.0 * u)
    t = np.fft.irfft(c * W, n=W, axis=-1) * scale
    f = np.fft.irfft(d * W, n=W, axis=-1) * scale
    if offset:
        t, f = t + OFFSET, f + OFFSET
    return torch.from_numpy(f.astype(np.float32)), torch.from_numpy(t.astype(np.float32))


def check_design(f, t, wb):
    """the fp64 oracle on the (plain, not offset) inputs, before they are relied on: every power positive, ratio
    strictly inside (0, 1) for k >= 1 and coherence for 1 <= k < K (at k = K it is in (0, 1])"""
    S = band_spectra(f, t, wb).sum(axis=0)
    assert (S[..., :2] > 0).all()
    ratio = S[..., 1:, 0] / S[..., 1:, 1]
    coh = S[..., 1:, 2] / np.sqrt(S[..., 1:, 0] * S[..., 1:, 1])
    assert 0.002 < ratio.min() and ratio.max() < 0.8, (ratio.min(), ratio.max())
    assert 0.1 < coh.min() and coh.max() <= 1.0 + 1e-12, (coh.min(), coh.max())
    assert coh.shape[-1] == 1 or coh[..., :-1].max() < 0.98, coh[..., :-1].max()
    return ratio, coh


def cos_weights(H):
    """(lat_deg, cos(latitude)) of an equiangular grid without pole rows (float64)"""
    lat = -90.0 + 90.0 / H + (180.0 / H) * np.arange(H)
    return lat, np.cos(np.deg2rad(lat))
