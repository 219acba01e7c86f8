"""SEEPS, the stable equitable error in probability space (Rodwell et al. 2010): did the forecast put dry, light and
heavy precipitation where they fell, measured against what is usual at each place?  Per lead time, channel and latitude
band the score, its split by the truth's category, the 3x3 table of (forecast category, truth category) and how much of
the grid took part, accumulated on the device.

The definitions are the project's own restatement of the published formulas, in the spirit of WeatherBench-2's SEEPS;
they are NOT pinned against any package.  The tests pin the kernel against a plain numpy restatement
(tests/seeps_oracle.py): the integers bit for bit, the double row sums within the rounding of a reordered double sum of
the same terms, and a single cell's score bit for bit.

Conventions.  Forecast ``f`` and truth ``o`` are ``[B, C, H, W]`` fp32 in physical units, in the chunk layout of
``forecast.postprocess`` (``PostSpec.names``).  The climatology (``climatology.build_seeps``) gives per slot, channel and
cell ``p1``, the climatological probability of a dry cell, and ``thr``, the edge between light and heavy; ``dry`` is its
``dry_threshold``.  Per cell, with the climatology of slot ``clim_index[b]``::

    cat(x) = 0 (dry) if x < dry, else 2 (heavy) if x >= thr, else 1 (light)       exact fp32 comparisons, no arithmetic

A cell is VALID iff ``f``, ``o``, ``p1`` and ``thr`` are finite, ``p_lo <= p1 <= p_hi`` (``p1_bounds``, rounded to fp32 and
compared in fp32; SEEPS is not defined where it is nearly always or nearly never dry) and the slot is in ``[0, K)``.  It
is MASKED iff all four are finite and the slot is in range, but ``p1`` is outside the bounds.  ANYTHING ELSE IS COUNTED
NOWHERE (as in ``events.EventTable``: a count cannot carry a NaN).  Per valid cell, in double, uncontracted, with ``p =
double(p1)``::

    a = 1.0 / (1.0 - p);  b = 1.0 / p;  c = 3.0 / (2.0 + p)
    M[cf][co] = [[0, a, 4.0*a], [b, 0, 3.0*a], [b + c, c, 0]]        (row: forecast category, column: truth category)
    s = 0.5 * M[cat(f)][cat(o)]

A constant forecast scores exactly 1 in expectation under the climatological frequencies ``(p, 2(1-p)/3, (1-p)/3)``, a
perfect forecast 0.

The device keeps, per (lead, chosen channel, latitude row ``h``), the integers ``{n[cf][co], n_masked}`` and the doubles
``S[co]``: the sum of ``s`` over the valid cells whose truth has category ``co`` - the score's usual decomposition; the
total is their sum, taken on the host.  Weights never enter the kernel: ``result`` applies the band and latitude weights
``wb[r, h]`` on the host, in numpy float64.  With ``nV = sum n[cf][co]``, ``N = sum_h wb nV``::

    seeps         = sum_h wb (S[0] + S[1] + S[2]) / N              seeps_skill = 1 - seeps
    by_truth[co]  = sum_h wb S[co] / N                             (sums to seeps)
    categories    = sum_h wb n[cf][co] / N                         forecast_freq / truth_freq: its row / column sums
    coverage      = N / (N + sum_h wb n_masked)

NaN where a denominator is 0.

Three launches per ``update`` (``csrc/seeps.hip``) read only the planes of the chosen channels, once.

No CPU fallback: ``update`` needs tensors on the HIP device.  Everything else (argument checks, ``counts``, ``result``,
``table``) works on any device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr
from ._leadtable import LeadTable, read
from ._tables import batch_stride, workspace

REAL_FIELDS = 3          # the sums of s by truth category {dry, light, heavy}
INT_FIELDS = 10          # {n[cf][co] (cf-major), n_masked}
CATEGORIES = ("dry", "light", "heavy")


def max_channels() -> int:
    return int(_lib.lib.paradis_seeps_max_channels())


def report(real: np.ndarray, ints: np.ndarray, n: np.ndarray, band_w: np.ndarray, names, bands) -> dict:
    """``real`` double ``[n_leads, Cs, H, 3]``, ``ints`` int64 ``[n_leads, Cs, H, 10]``, ``n`` ``[n_leads]`` and the band
    weights ``[R, H]`` -> the reported values (``SeepsTable.result``).  Host only."""
    wb = np.asarray(band_w, np.float64)
    ints = np.asarray(ints)
    table = ints[..., :9].astype(np.float64)
    N = np.einsum("rh,lch->lcr", wb, table.sum(axis=-1))
    S = np.einsum("rh,lchk->lcrk", wb, np.asarray(real, np.float64))
    cat = np.einsum("rh,lchk->lcrk", wb, table)
    masked = np.einsum("rh,lch->lcr", wb, ints[..., 9].astype(np.float64))
    never = np.asarray(n).reshape(-1, 1, 1) == 0
    with np.errstate(all="ignore"):
        Nn = np.where(never | (N == 0), np.nan, N)
        seen = np.where(never | (N + masked == 0), np.nan, N + masked)
        seeps = ((S[..., 0] + S[..., 1]) + S[..., 2]) / Nn
        categories = (cat / Nn[..., None]).reshape(cat.shape[:-1] + (3, 3))
        res = {"seeps": seeps, "seeps_skill": 1.0 - seeps, "by_truth": S / Nn[..., None], "categories": categories,
               "forecast_freq": categories.sum(axis=-1), "truth_freq": categories.sum(axis=-2), "coverage": N / seen}
    res["count"] = np.asarray(n).copy()
    res["names"] = list(names)
    res["bands"] = list(bands)
    return res


class SeepsTable(LeadTable):
    """Per-lead SEEPS of a rollout, accumulated on the device (module docstring for the formulas; the project's own
    definitions, not pinned against any package; cells that are not valid add nothing, unlike ``Scorecard``, where NaN
    propagates).

    ``names``: the chunk's channel names (``PostSpec.names``); ``lat_deg``: ``[H]`` latitudes in degrees; ``climatology``:
    a ``climatology.SeepsClimatology`` on ``device`` (default: where its ``data`` lives) - ``dry_threshold`` is taken
    from it; ``channels``: the precipitation channels to score (default the climatology's names, at most
    ``paradis_seeps_max_channels()``), each among ``names`` and among the climatology's names - only these planes are
    read; ``all_names`` stays the state's names, ``names`` the subset; with the climatology's own names in their order
    its ``data`` is read in place, another choice is gathered once, here; ``p1_bounds``: ``(p_lo, p_hi)``, ``0 < p_lo <=
    p_hi < 1``, rounded to fp32; ``bands`` and ``weights`` as in ``spectrum.Spectra``: a dict name -> ``(lat_lo,
    lat_hi)`` in degrees, inclusive (default ``{"global": (-90, 90)}``), row weights ``weights[h]`` inside a band and 0
    outside (default ``cos(lat)``, pole rows 0).

    The accumulators live on ``device``: ``acc_real`` double ``[n_leads, Cs, H, 3]``, ``acc_int`` int64 ``[n_leads, Cs,
    H, 10]`` and ``n_samples`` int64 ``[n_leads]`` - 104 bytes per lead, channel and row.

    ``update(lead, forecast, truth, clim_index=None)``: three launches on the current stream, no host synchronisation,
    graph-capturable, no input is written; ``forecast`` / ``truth`` ``[B, C, H, W]`` fp32 with dense ``[C, H, W]`` states
    and any batch stride; ``clim_index`` ``[B]`` int32 on the device (optional with a one-slot climatology); a sample
    whose slot is outside ``[0, K)`` adds nothing but its count.  ``counts(sync_dist=False)``: the raw accumulators,
    ``sums [n_leads, Cs, H, 3]`` float64, ``table [n_leads, Cs, H, 3, 3]`` and ``masked [n_leads, Cs, H]`` int64,
    ``n_samples [n_leads]``.  ``result(sync_dist=False)``: one device read (after ONE all-reduce with ``sync_dist``; the
    integers travel as doubles, exact below 2^53); float64 ``seeps``, ``seeps_skill`` and ``coverage`` ``[n_leads, Cs,
    R]``, ``by_truth``, ``forecast_freq`` and ``truth_freq`` ``[n_leads, Cs, R, 3]``, ``categories [n_leads, Cs, R, 3,
    3]`` (forecast category, truth category), ``count [n_leads]``, ``names`` (the chosen channels) and ``bands``; NaN
    where nothing was valid and for leads never updated.  ``table(result, channel, band=...)``: plain text for logs.
    ``reset()`` clears the accumulators."""

    IT = "the table"
    IT_HAS = "the table has"
    NOUN = "the SEEPS table"
    HAS = "the SEEPS table has"
    NEEDS = "a SEEPS table needs"
    TAKES_CLIM_INDEX = True
    members = 1

    def __init__(self, names: Sequence[str], lat_deg, n_leads: int, climatology, *,
                 channels: Optional[Sequence[str]] = None, p1_bounds=(0.1, 0.85), bands: Optional[dict] = None,
                 weights=None, device=None):
        from .climatology import SeepsClimatology
        if not isinstance(climatology, SeepsClimatology):
            raise ValueError("SeepsTable: climatology must be a climatology.SeepsClimatology (climatology.build_seeps)")
        data = climatology.data
        super().__init__(names, n_leads, data.device if device is None else device)
        self._set_grid(lat_deg, weights, bands)
        self._set_channels(climatology.names if channels is None else channels)
        if len(self.names) > max_channels():
            raise ValueError(f"SeepsTable: {len(self.names)} channels, at most {max_channels()} go into one table")
        for c in self.names:
            if c not in climatology.names:
                raise ValueError(f"SeepsTable: no SEEPS climatology was built for channel '{c}'")
        try:
            p_lo, p_hi = (float(np.float32(v)) for v in p1_bounds)
        except (TypeError, ValueError):
            raise ValueError(f"SeepsTable: p1_bounds must be (p_lo, p_hi), got {p1_bounds!r}") from None
        if not (0.0 < p_lo <= p_hi < 1.0):
            raise ValueError(f"SeepsTable: p1_bounds must satisfy 0 < p_lo <= p_hi < 1, got {p1_bounds!r}")
        self.p1_bounds = (p_lo, p_hi)
        self.dry_threshold = climatology.dry_threshold
        if data.shape[1] < 1 or data.shape[3] != self.H:
            raise ValueError(f"SeepsTable: the climatology is {tuple(data.shape)}, the table has {self.H} latitudes and "
                             f"needs at least one slot")
        if data.device.type != self.device.type:
            raise ValueError(f"SeepsTable: climatology lives on {data.device}, the table on {self.device}")
        self.W = int(data.shape[4])
        if data.stride(4) != 1 or data.stride(3) != self.W:
            raise ValueError("SeepsTable: the climatology's planes must be dense [H, W]")
        if self.names != climatology.names:                  # (another choice or order of channels: gathered once)
            with torch.inference_mode(False):
                data = data[:, :, [climatology.names.index(c) for c in self.names]].contiguous()
        self.seeps_climatology, self._data = climatology, data
        self.climatology = data[0]                           # p1 [K, Cs, H, W]: what the shared clim_index checks look at
        self._chan = np.ascontiguousarray(self.index, np.int32)      # host: travels as kernel arguments
        Cs = len(self.names)
        with torch.inference_mode(False):
            self.acc_real = torch.zeros(self.n_leads, Cs, self.H, REAL_FIELDS, dtype=torch.float64, device=self.device)
            self.acc_int = torch.zeros(self.n_leads, Cs, self.H, INT_FIELDS, dtype=torch.int64, device=self.device)
            self.n_samples = torch.zeros(self.n_leads, dtype=torch.int64, device=self.device)

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor,
               clim_index: Optional[torch.Tensor] = None) -> None:
        B, C, H, W = self._check(lead, forecast, truth, clim_index, n_lon=self.W)
        require_hip(forecast, truth)
        if not self.acc_real.is_cuda:
            raise RuntimeError("SeepsTable.update: the table was made with a CPU device (there is no CPU fallback)")
        if B == 0:             # (empty tensors have no address to hand over; the entry point would do nothing either)
            return
        idx, K = self._clim_args(clim_index, forecast)
        data, Cs, P = self._data, len(self.names), H * W
        lead = int(lead)
        ws = workspace(self._ws, forecast.device, int(_lib.lib.paradis_seeps_ws_bytes(B, Cs, H, W)))
        _lib.call("seeps_update", 16.0 * B * Cs * P, dptr(forecast), batch_stride(forecast, C * P), dptr(truth),
                  batch_stride(truth, C * P), dptr(data[0]), dptr(data[1]), data.stride(1), data.stride(2), dptr(idx), K,
                  self._chan.ctypes.data, Cs, self.dry_threshold, self.p1_bounds[0], self.p1_bounds[1],
                  dptr(self.acc_real[lead]), dptr(self.acc_int[lead]), dptr(self.n_samples[lead:]), dptr(ws), B, C, H, W,
                  stream_ptr())

    def reset(self) -> None:
        self.acc_real.zero_()
        self.acc_int.zero_()
        self.n_samples.zero_()

    def _read(self, sync_dist: bool):
        """one device read: ``(real, ints, n_samples)`` - the integers go behind the doubles as doubles (exact below
        2^53), so that ONE all-reduce sums both (``EnsembleCard._read``'s way)"""
        flat = torch.cat([self.acc_real.reshape(-1), self.acc_int.reshape(-1).double()])
        a, n = read(flat, self.n_samples.double(), sync_dist)
        nr = self.acc_real.numel()
        real = a[:nr].reshape(tuple(self.acc_real.shape)).copy()
        ints = np.rint(a[nr:]).astype(np.int64).reshape(tuple(self.acc_int.shape))
        return real, ints, np.rint(n).astype(np.int64)

    def counts(self, sync_dist: bool = False) -> dict:
        real, ints, n = self._read(sync_dist)
        return {"sums": real, "table": ints[..., :9].reshape(ints.shape[:-1] + (3, 3)).copy(),
                "masked": ints[..., 9].copy(), "n_samples": n}

    def result(self, sync_dist: bool = False) -> dict:
        real, ints, n = self._read(sync_dist)
        return report(real, ints, n, self.band_w, self.names, self.bands)

    @staticmethod
    def table(result: dict, channel: str, band: Optional[str] = "global") -> str:
        """plain text: a row per lead with ``count``, the scores, the split by the truth's category and the coverage,
        then a row per lead of the 3x3 joint frequencies, forecast category major (``band=None``: the first band)"""
        names: List[str] = list(result["names"])
        bands: List[str] = list(result["bands"])
        if str(channel) not in names:
            raise ValueError(f"SeepsTable.table: channel '{channel}' is not among the table's names")
        band = bands[0] if band is None else str(band)
        if band not in bands:
            raise ValueError(f"SeepsTable.table: band '{band}' is not among the table's bands")
        c, r = names.index(str(channel)), bands.index(band)
        heads = ("seeps", "seeps_skill") + tuple(f"truth_{k}" for k in CATEGORIES) + ("coverage",)
        lines = [f"{channel} / {band}"]
        lines.append(f"{'lead':<6}{'count':>8}" + "".join(f"{m:>14}" for m in heads))
        n_leads = len(result["count"])
        for lead in range(n_leads):
            vals = [result["seeps"][lead, c, r], result["seeps_skill"][lead, c, r]]
            vals += [result["by_truth"][lead, c, r, k] for k in range(3)] + [result["coverage"][lead, c, r]]
            lines.append(f"{lead:<6d}{int(result['count'][lead]):>8d}" + "".join(f"{v:>14.5g}" for v in vals))
        lines.append("")
        pairs = [f"{a[0]}->{b[0]}" for a in CATEGORIES for b in CATEGORIES]       # forecast -> truth: d->d, d->l, ..
        lines.append(f"{'f->o':<6}{'count':>8}" + "".join(f"{p:>8}" for p in pairs))
        for lead in range(n_leads):
            vals = "".join(f"{result['categories'][lead, c, r, i, j]:>8.4f}" for i in range(3) for j in range(3))
            lines.append(f"{lead:<6d}{int(result['count'][lead]):>8d}" + vals)
        return "\n".join(lines)
