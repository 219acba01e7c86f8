"""Zonal power spectra of forecast and truth per lead time: at which scales a forecast has gone wrong - the blurring
curve ``ratio``, the ``coherence`` and the ``error_power`` per zonal wavenumber, accumulated on the device.

The definition is the project's own, in the spirit of WeatherBench-2's ``ZonalEnergySpectrum``; it is NOT pinned
against WeatherBench-2 (which no build machine of this project holds).  The tests pin the kernel against a plain numpy
fp64 restatement of the formulas below (tests/spectrum_oracle.py).

Conventions.  Forecast ``f`` and truth ``t`` are ``[B, C, H, W]`` fp32 in physical units, in the chunk layout of
``forecast.postprocess``; ``W`` even, ``K = W / 2``, ``k = 0 .. K``.  Per row ``h`` of a plane::

    X[h,k]  = (1/W) sum_i x[h,i] exp(-2 pi i k i / W)          m_k = 1 for k in {0, K}, else 2
    pf[h,k] = m_k |F[h,k]|^2      pt[h,k] = m_k |T[h,k]|^2      co[h,k] = m_k Re(F[h,k] conj T[h,k])

so that ``sum_k pf[h,k] = mean_i f[h,i]^2`` (Parseval).  Bands ``r = 0 .. R-1`` carry row weights ``wb[r,h] >= 0``, not
all zero in any band::

    S_ff[r,k] = sum_h wb[r,h] pf[h,k] / sum_h wb[r,h]          (S_tt from pt, S_ft from co)

A row with ``wb[r,h] == 0`` is left out of band ``r`` - not multiplied in, so a NaN in it never reaches the band - and a
row of weight zero in every band is neither read nor transformed.  Otherwise non-finite values are NOT masked: they
propagate, as in ``verify.Scorecard`` - a non-finite value in either field of a row reaches all three sums of every band
that holds the row (forecast and truth rows share one transform).  Accumulated per (lead, channel, band, k), three
doubles ``{sum S_ff, sum S_tt, sum S_ft}`` over the samples, and a ``count`` per lead.  Reported: ``power_forecast``,
``power_truth``, ``cospectrum`` (sum / count), ``ratio = S_ff / S_tt``, ``coherence = S_ft / sqrt(S_ff S_tt)`` and
``error_power = S_ff + S_tt - 2 S_ft``, the spectrum of ``f - t``: with the band weights equal to a scorecard's latitude
weights, ``sum_k error_power`` is that scorecard's ``rmse^2``.

One launch pair per ``update`` (``csrc/spectrum.hip``): forecast and truth rows go through one complex fp32 transform in
LDS (a mixed-radix FFT where ``W`` is a product of 2, 3 and 5, a direct row DFT for other small even ``W``), relative to
a per-row pivot that keeps a large mean out of the fp32 arithmetic; everything after the transform is double, summed in
a fixed order.  The twiddle table is built here once, in double, and rounded to fp32.

No CPU fallback: ``update`` needs tensors on the HIP device.  The host side (argument checks, ``result``,
``effective_resolution``, ``table``) works on any device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr
from ._leadtable import LeadTable, band_weights, read          # noqa: F401  (band_weights: importable from here)
from ._tables import batch_stride, workspace

ACC_FIELDS = 3          # {sum S_ff, sum S_tt, sum S_ft}
QUANTITIES = ("power_forecast", "power_truth", "cospectrum", "ratio", "coherence", "error_power")
SCHEDULES = {0: None, 1: "fft", 2: "direct"}


def lat_weights_from(loss) -> torch.Tensor:
    """the latitude weights of a ``ParadisLoss`` (``loss.lat_weights_buf``), as ``Spectra`` takes them"""
    return loss.lat_weights_buf


def schedule(W: int) -> Optional[str]:
    """``"fft"``, ``"direct"`` or ``None`` (refused): the kernel schedule of a row of ``W`` longitudes"""
    return SCHEDULES[int(_lib.lib.paradis_spectrum_schedule(int(W)))]


def twiddle_table(W: int) -> np.ndarray:
    """``exp(-2 pi i j / W)``, ``j < W``, as float32 ``[W, 2]``: computed in double, rounded once"""
    ang = -2.0 * np.pi * np.arange(int(W), dtype=np.float64) / float(W)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)


class Spectra(LeadTable):
    """Per-lead zonal power spectra of a rollout and its truth, accumulated on the device (module docstring for the
    formulas; the project's own definition, not pinned against WeatherBench-2).

    ``names``: the chunk's channel names (``PostSpec.names``); ``lat_deg``: ``[H]`` latitudes in degrees; ``bands``: a
    dict name -> ``(lat_lo, lat_hi)`` in degrees, inclusive (default ``{"global": (-90, 90)}``), each band's row weights
    being ``weights[h]`` inside the band and 0 outside; ``weights``: ``[H]`` (any shape with H entries; default
    ``cos(lat)``; ``Spectra.lat_weights_from(loss)`` is accepted); ``channels``: the subset of ``names`` to analyse
    (default all) - only these planes are read.  ``acc`` is the double ``[n_leads, Cs, R, K + 1, 3]`` accumulator on
    ``device``, ``n_leads * Cs * R * (K + 1) * 24`` bytes: with every one of 96 channels at 721 x 1440 that is 6.6 MB
    per lead and band, which is what ``channels=`` is for; ``count`` is double ``[n_leads]``.

    ``update(lead, forecast, truth)``: one launch pair on the current stream, no host synchronisation, neither input is
    written; ``forecast`` / ``truth`` ``[B, C, H, W]`` fp32 with dense ``[C, H, W]`` states and any batch stride
    (``chunk[:, slot]`` and ``truth[:, k]`` are consumed in place).  ``W`` must be even and either a product of 2, 3
    and 5 up to ``paradis_spectrum_fft_max_w()`` or at most ``paradis_spectrum_direct_max_w()``.
    ``result(sync_dist=False)``: one device read; the six ``QUANTITIES`` as numpy float64 ``[n_leads, Cs, R, K + 1]``,
    ``"wavenumber"`` ``[K + 1]``, ``"count"`` ``[n_leads]``, ``"names"`` (the chosen channels) and ``"bands"``; leads
    never updated come back as NaN with count 0.  With ``sync_dist=True`` and an initialised process group the
    accumulators are summed over the ranks by ONE all-reduce first (through the host under gloo).
    ``reset()`` clears the accumulators.  ``bind(W)`` makes them ahead of the first ``update`` (which otherwise does
    it: the number of longitudes is not a constructor argument).  ``effective_resolution(result, threshold=0.5)`` and
    ``table(result, channel, band=...)`` are host-only."""

    IT = NOUN = "the spectra"
    IT_HAS = HAS = "the spectra have"
    NEEDS = "spectra need"
    TAKES_CLIM_INDEX = False

    def __init__(self, names: Sequence[str], lat_deg, n_leads: int, *, bands: Optional[dict] = None, weights=None,
                 channels: Optional[Sequence[str]] = None, device="cuda"):
        super().__init__(names, n_leads, device)
        self._set_grid(lat_deg, weights, bands)
        self._set_channels(channels)
        with torch.inference_mode(False):
            self._band_w = torch.from_numpy(self.band_w).to(self.device)
            self._band_wsum = torch.from_numpy(self.band_w.sum(axis=1)).to(self.device)
            self._chan = None if channels is None else torch.tensor(self.index, dtype=torch.int32, device=self.device)
            self.count = torch.zeros(self.n_leads, dtype=torch.float64, device=self.device)
        self.acc: Optional[torch.Tensor] = None       # [n_leads, Cs, R, K + 1, 3] once W is known (first update)

    lat_weights_from = staticmethod(lat_weights_from)

    def bind(self, W: int) -> None:
        """makes the accumulator and the twiddle table for ``W`` longitudes; the first ``update`` does it by itself"""
        if isinstance(W, bool) or int(W) != W or schedule(int(W)) is None:
            raise ValueError(f"Spectra.bind: {W!r} longitudes are refused: W must be even and either a product of 2, 3 "
                             f"and 5 up to {_lib.lib.paradis_spectrum_fft_max_w()} or at most "
                             f"{_lib.lib.paradis_spectrum_direct_max_w()}")
        if self.W is not None and int(W) != self.W:
            raise ValueError(f"Spectra.bind: the spectra are bound to {self.W} longitudes already")
        if self.acc is not None:
            return
        W = int(W)
        with torch.inference_mode(False):
            self.acc = torch.zeros(self.n_leads, len(self.names), len(self.bands), W // 2 + 1, ACC_FIELDS,
                                   dtype=torch.float64, device=self.device)
            self._tw = torch.from_numpy(twiddle_table(W)).to(self.device)
        self.W = W

    def _check_longitudes(self, W: int) -> None:
        if self.W is not None and W != self.W:
            raise ValueError(f"Spectra.update: forecast has {W} longitudes, earlier updates had {self.W}")
        if schedule(W) is None:
            raise ValueError(f"Spectra.update: {W} longitudes are refused: W must be even and either a product of 2, 3 "
                             f"and 5 up to {_lib.lib.paradis_spectrum_fft_max_w()} or at most "
                             f"{_lib.lib.paradis_spectrum_direct_max_w()}")

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor) -> None:
        B, C, H, W = self._check(lead, forecast, truth)
        require_hip(forecast, truth)
        if not self._band_w.is_cuda:
            raise RuntimeError("Spectra.update: the spectra were made with a CPU device (there is no CPU fallback)")
        if B == 0:             # (empty tensors have no address to hand over; the entry point would do nothing either)
            return
        if self.acc is None:
            self.bind(W)
        Cs, R = len(self.names), len(self.bands)
        ws = workspace(self._ws, forecast.device, int(_lib.lib.paradis_spectrum_ws_bytes(B, Cs, H, W, R)))
        _lib.call("spectrum_update", 8.0 * B * Cs * H * W, dptr(forecast), batch_stride(forecast, C * H * W),
                  dptr(truth), batch_stride(truth, C * H * W), dptr(self._chan), Cs, dptr(self._band_w),
                  dptr(self._band_wsum), dptr(self._tw), dptr(self.acc[int(lead)]), dptr(self.count[int(lead):]),
                  dptr(ws), B, C, H, W, R, stream_ptr())

    def reset(self) -> None:
        self.count.zero_()
        if self.acc is not None:
            self.acc.zero_()

    def result(self, sync_dist: bool = False) -> dict:
        if self.acc is None:
            raise RuntimeError("Spectra.result: no update yet - the number of longitudes is not known")
        return report(*read(self.acc, self.count, sync_dist), self.names, self.bands)

    @staticmethod
    def effective_resolution(result: dict, threshold: float = 0.5) -> np.ndarray:
        """int64 ``[n_leads, Cs, R]``: the first wavenumber ``k >= 1`` whose ``ratio`` is below ``threshold`` - the
        scale from which on the forecast holds less than that share of the truth's power -, ``K + 1`` if there is none
        (a NaN ratio is not below anything)"""
        ratio = np.asarray(result["ratio"])
        K1 = ratio.shape[-1]
        below = ratio[..., 1:] < float(threshold)
        first = np.argmax(below, axis=-1) + 1
        return np.where(below.any(axis=-1), first, K1).astype(np.int64)

    @staticmethod
    def table(result: dict, channel: str, band: Optional[str] = None, wavenumbers: Optional[Sequence[int]] = None) -> str:
        """plain text, one block per quantity out of ``power_truth``, ``ratio``, ``coherence``: a row per lead, a
        column per wavenumber (``wavenumbers``: default 1, 2, 4, .. and K)"""
        names: List[str] = list(result["names"])
        bands: List[str] = list(result["bands"])
        if str(channel) not in names:
            raise ValueError(f"Spectra.table: channel '{channel}' is not among the spectra's names")
        band = bands[0] if band is None else str(band)
        if band not in bands:
            raise ValueError(f"Spectra.table: band '{band}' is not among the spectra's bands")
        c, r = names.index(str(channel)), bands.index(band)
        K = len(result["wavenumber"]) - 1
        if wavenumbers is None:
            ks = sorted({min(2 ** j, K) for j in range(K.bit_length() + 1)} | {K})
        else:
            ks = [int(k) for k in wavenumbers]
            for k in ks:
                if not 0 <= k <= K:
                    raise ValueError(f"Spectra.table: wavenumber {k} is outside [0, {K}]")
        lines = [f"{channel} / {band}"]
        for q in ("power_truth", "ratio", "coherence"):
            lines.append(f"{q:<12}{'count':>8}" + "".join(f"{'k=' + str(k):>12}" for k in ks))
            for lead in range(result[q].shape[0]):
                vals = "".join(f"{result[q][lead, c, r, k]:>12.4e}" for k in ks)
                lines.append(f"{lead:<12d}{int(result['count'][lead]):>8d}" + vals)
            lines.append("")
        return "\n".join(lines[:-1])


def report(a: np.ndarray, n: np.ndarray, names, bands) -> dict:
    """``a`` double ``[n_leads, Cs, R, K + 1, 3]`` and ``n`` ``[n_leads]`` -> the reported values (``Spectra.result``)"""
    cnt = n.reshape(-1, 1, 1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ff, tt, ft = a[..., 0] / cnt, a[..., 1] / cnt, a[..., 2] / cnt
        res = {"power_forecast": ff, "power_truth": tt, "cospectrum": ft, "ratio": ff / tt,
               "coherence": ft / np.sqrt(ff * tt), "error_power": ff + tt - 2.0 * ft}
    for q in QUANTITIES:
        res[q] = np.where(cnt > 0, res[q], np.nan)            # leads never updated
    res["wavenumber"] = np.arange(a.shape[3])
    res["count"] = n.copy()
    res["names"] = list(names)
    res["bands"] = list(bands)
    return res
