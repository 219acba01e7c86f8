"""Neighbourhood verification: at which scale does the forecast become skilful?  The fractions skill score (FSS, Roberts
and Lean 2008) per lead time, event source, latitude band, scale and threshold: instead of asking whether forecast and
truth put an event into the same cell (``events.EventTable``, which punishes a good high-resolution forecast twice for
a small displacement), it compares the NUMBER of event cells in a window around each cell.

The definitions are the project's own, textbook formulas; they are NOT pinned against any package.  The tests pin the
kernel against a plain numpy restatement (tests/fss_oracle.py) - exactly: everything after the threshold decision is
an integer, so the device result equals the restatement bit for bit.

Events.  Sources, thresholds, directions and validity are exactly ``events.EventTable``'s (its module docstring): per
cell and threshold ``j`` the bits ``F[j]`` (forecast event) and ``O[j]`` (truth event).  AN INVALID CELL IS A NON-EVENT
IN BOTH FIELDS here (``F = O = 0``): a window has no hole; ``nV`` and ``valid_fraction`` report how many cells were
valid.

Scales and windows.  Scale ``k`` has a latitude half-width ``ny[k] >= 0`` in rows (``scales``) and a longitude half-width
``nx[k][h] >= 0`` in cells per centre row ``h``, ``2 nx + 1 <= W``.  The window of centre cell ``(h, w)`` is the
rectangle of rows ``max(0, h - ny) .. min(H - 1, h + ny)`` - clipped at the grid edge, no over-the-pole wrap - and
columns ``w - nx[k][h] .. w + nx[k][h]`` modulo ``W``.  ``lon_scaling``::

    "cells"    nx[k][h] = min(ny[k], cap)                                      cap = min(max_half_x, (W - 1) // 2)
    "metric"   nx[k][h] = min(floor(ny[k] * dlat / (dlon * cos(lat_h)) + 0.5), cap),  dlat = |lat[1] - lat[0]|,
               dlon = 360 / W; pole rows (cos(lat) <= 0) take the cap; ny = 0 gives nx = 0 in every row: the window is
               about as wide in km at every latitude as it is high

or an explicit integer table ``half_x [K, H]`` (refused when an entry is outside ``[0, cap]``).

Sums.  ``cF`` / ``cO``: the number of ``F`` / ``O`` bits in the window.  The device keeps per (lead, source ``s``, centre
row ``h``) ``nV``, ``nF[j]``, ``nO[j]`` - ``EventTable``'s - and per scale ``k`` and threshold ``j`` the sums over the
row's cells ``FF = sum_w cF^2``, ``OO = sum_w cO^2``, ``FO = sum_w cF cO``, all int64, accumulated over samples and
updates: ``acc [n_leads, S, H, 1 + 2 TMAX + 3 K_MAX TMAX]`` (the layout of ``paradis_fss_update``).  Weights never
enter the kernel; ``result`` works on the host in numpy float64, with the window size ``N[k][h] = (rows in the
window) (2 nx[k][h] + 1)`` and the band / latitude weights ``wb[r][h]`` of ``spectrum.band_weights``::

    fbs     = sum_h wb (FF + OO - 2 FO) / N^2            fbs_ref = sum_h wb (FF + OO) / N^2
    fss     = 1 - fbs / fbs_ref                          (NaN where fbs_ref == 0)
    base_rate = sum_h wb nO / sum_h wb nV                frequency_bias = sum_h wb nF / sum_h wb nO
    fss_uniform = 0.5 + base_rate / 2

(``fbs`` and ``fbs_ref`` are weighted sums, not means: their ratio is what counts.)  ``skilful_scale`` gives the first
scale, in the given order, with ``fss >= fss_uniform``; it plays the part ``effective_resolution()`` plays for
``Spectra``.

Three launches per ``update`` (``csrc/fss.hip``); only the planes of the chosen sources are read, once.

No CPU fallback: ``update`` needs tensors on the HIP device.  Everything else works on any device.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr
from .events import EventLeadTable, _ratio, lookup, parse_events          # noqa: F401  (parse_events: importable from here)

WHO = "FractionsTable"


def limits() -> dict:
    """the limits of ``csrc/fss.hip``"""
    L = _lib.lib
    return {"max_scales": int(L.paradis_fss_max_scales()), "max_half_y": int(L.paradis_fss_max_half_y()),
            "max_half_x": int(L.paradis_fss_max_half_x()), "max_w": int(L.paradis_fss_max_w())}


def half_x_cap(W: int) -> int:
    return min(limits()["max_half_x"], (int(W) - 1) // 2)


def half_x_table(scales: Sequence[int], lat_deg, W: int, lon_scaling: str = "cells") -> np.ndarray:
    """int32 ``[K, H]`` longitude half-widths of ``lon_scaling`` (module docstring)"""
    lat = np.asarray(lat_deg, np.float64).reshape(-1)
    ny = np.asarray(list(scales), np.int64).reshape(-1)
    cap = half_x_cap(W)
    if lon_scaling == "cells":
        nx = np.repeat(np.minimum(ny, cap)[:, None], lat.size, axis=1)
    elif lon_scaling == "metric":
        if lat.size < 2:
            raise ValueError(f"{WHO}: lon_scaling='metric' needs at least two latitudes")
        dlat, dlon = abs(lat[1] - lat[0]), 360.0 / W
        c = np.cos(np.deg2rad(lat))
        c[np.abs(lat) == 90.0] = 0.0                                    # (cos(+-90 deg) in double is 6e-17, not 0)
        pole = c <= 0.0
        with np.errstate(all="ignore"):
            x = np.floor(ny[:, None] * dlat / (dlon * np.where(pole, 1.0, c))[None, :] + 0.5)
        nx = np.where(pole[None, :], cap, np.minimum(x, cap)).astype(np.int64)
        nx[ny == 0] = 0
    else:
        raise ValueError(f"{WHO}: lon_scaling must be 'cells' or 'metric', got {lon_scaling!r}")
    return np.ascontiguousarray(nx.astype(np.int32))


def window_cells(scales: Sequence[int], half_x: np.ndarray, H: int) -> np.ndarray:
    """int64 ``[K, H]``: the cells of the window centred in row ``h`` - its rows inside the grid times ``2 nx + 1``"""
    h = np.arange(H)[None, :]
    ny = np.asarray(list(scales), np.int64)[:, None]
    rows = np.minimum(H - 1, h + ny) - np.maximum(0, h - ny) + 1
    return rows * (2 * np.asarray(half_x, np.int64) + 1)


def skilful_scale(result: dict) -> np.ndarray:
    """int64 ``[n_leads, S, R, T]``: the index of the first scale, in the given order, with ``fss >= fss_uniform``; -1 if
    there is none (or the entry is NaN)"""
    with np.errstate(all="ignore"):
        ok = result["fss"] >= result["fss_uniform"][:, :, :, None, :]                  # [L, S, R, K, T]
    first = np.argmax(ok, axis=3)
    return np.where(ok.any(axis=3), first, -1).astype(np.int64)


class FractionsTable(EventLeadTable):
    """Per-lead fractions skill scores over several window sizes, their integer sums accumulated on the device (module
    docstring for the definitions; an invalid - non-finite - cell is a non-event in both fields).

    ``names``, ``lat_deg``, ``n_leads``, ``events``, ``bands``, ``weights``, ``climatology``: as ``events.EventTable``.
    ``n_lon``: the number of longitudes ``W``.  ``scales``: 1 to ``paradis_fss_max_scales()`` latitude half-widths in
    rows, each in ``[0, paradis_fss_max_half_y()]``, e.g. ``[0, 1, 2, 4, 8, 16]``.  ``lon_scaling`` / ``half_x``: the
    longitude half-widths (module docstring); ``self.half_x`` is the int32 ``[K, H]`` table in use.

    ``acc`` is the int64 ``[n_leads, S, H, 1 + 2 TMAX + 3 K_MAX TMAX]`` accumulator on ``device`` (209 entries a row),
    ``n_samples`` int64 ``[n_leads]``.

    ``update(lead, forecast, truth, clim_index=None)``: three launches on the current stream, no host synchronisation,
    graph-capturable after a first eager call (which uploads ``half_x`` and sizes the workspace), neither input is
    written; the arguments are ``EventTable.update``'s.  What only the entry point
    can refuse (more than ``paradis_fss_max_w()`` longitudes) comes back as a ``ValueError``.
    ``counts(sync_dist=False)``: one device read (after ONE all-reduce with ``sync_dist``); the raw int64 arrays ``valid
    [n_leads, S, H]``, ``forecast_yes``, ``observed_yes`` ``[n_leads, S, H, T]``, ``ff``, ``oo``, ``fo`` ``[n_leads, S, H,
    K, T]`` (-1 past a source's own thresholds) and ``n_samples [n_leads]``.
    ``result(sync_dist=False)``: float64 ``fss``, ``fbs``, ``fbs_ref`` ``[n_leads, S, R, K, T]``, ``base_rate``,
    ``frequency_bias``, ``fss_uniform`` ``[n_leads, S, R, T]`` (NaN past a source's thresholds and for leads never
    updated), ``valid_fraction [n_leads, S, R]``, ``count [n_leads]``, ``labels``, ``thresholds``, ``directions``,
    ``bands``, ``scales`` and ``window_cells [K, H]``.  ``skilful_scale(result)``; ``table(result, label, band=None)``:
    plain text.  ``reset()`` clears the accumulators."""

    NOUN = "the fractions table"
    HAS = "the fractions table has"
    NEEDS = "a fractions table needs"

    def __init__(self, names: Sequence[str], lat_deg, n_lon: int, n_leads: int, events: dict, scales: Sequence[int],
                 lon_scaling: str = "cells", half_x=None, bands: Optional[dict] = None, weights=None,
                 climatology: Optional[torch.Tensor] = None, device="cuda"):
        lim = limits()
        self.kmax = lim["max_scales"]
        super().__init__(names, lat_deg, n_leads, events, bands, weights, climatology, device,
                         row=lambda tmax: 1 + 2 * tmax + 3 * self.kmax * tmax, n_lon=n_lon)
        H, lat = self.H, self.lat
        try:
            sc = [s for s in scales]
        except TypeError:
            raise ValueError(f"{WHO}: scales must be a list of latitude half-widths in rows") from None
        if not 1 <= len(sc) <= self.kmax:
            raise ValueError(f"{WHO}: {len(sc)} scales, 1 to {self.kmax} are allowed")
        for s in sc:
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) <= lim["max_half_y"]:
                raise ValueError(f"{WHO}: a scale must be an integer in [0, {lim['max_half_y']}] rows, got {s!r}")
        self.scales = [int(s) for s in sc]
        K, cap = len(self.scales), half_x_cap(self.W)
        if half_x is None:
            self.half_x = half_x_table(self.scales, lat, self.W, lon_scaling)
        else:
            hx = np.asarray(half_x.detach().cpu() if isinstance(half_x, torch.Tensor) else half_x)
            if hx.shape != (K, H) or hx.dtype.kind not in "iu":
                raise ValueError(f"{WHO}: half_x must be an integer table [{K}, {H}]")
            if (hx < 0).any() or (hx > cap).any():
                raise ValueError(f"{WHO}: half_x must lie in [0, {cap}] (2 nx + 1 <= W = {self.W}, at most "
                                 f"{lim['max_half_x']} cells)")
            self.half_x = np.ascontiguousarray(hx.astype(np.int32))
        self._half_y = np.ascontiguousarray(np.asarray(self.scales, np.int32))
        self.window_cells = window_cells(self.scales, self.half_x, H)
        self.head = 1 + 2 * self.tmax
        self._half_x_dev: Dict[str, torch.Tensor] = {}     # device -> half_x there

    def _check(self, lead, forecast, truth, clim_index):
        return super()._check(lead, forecast, truth, clim_index, n_lon=self.W)

    def _entry_tables(self, device) -> tuple:
        """``half_y`` on the host and ``half_x`` on ``device``, copied there at its first use"""
        dev = str(device)
        if dev not in self._half_x_dev:
            with torch.inference_mode(False):
                self._half_x_dev[dev] = torch.from_numpy(self.half_x).to(device)
        return self._half_y.ctypes.data, dptr(self._half_x_dev[dev])

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor,
               clim_index: Optional[torch.Tensor] = None) -> None:
        B, C, H, W = self._check(lead, forecast, truth, clim_index)
        S, K = len(self.labels), len(self.scales)
        try:
            self._launch("fss_update", _lib.lib.paradis_fss_ws_bytes(B, S, H, W, K), lead, forecast, truth, clim_index, B,
                         B, C, S, H, W, K)
        except RuntimeError as e:
            if "(code 1)" in str(e):               # an argument the entry point refused, before any HIP call
                raise ValueError(f"{WHO}.update: {_lib.last_error()}") from None
            raise

    def counts(self, sync_dist: bool = False) -> dict:
        a, n, out = self._counts_head(sync_dist)
        T, TM, K = self.T, self.tmax, len(self.scales)
        win = a[..., self.head:self.head + 3 * K * TM].reshape(a.shape[:3] + (K, TM, 3))[..., :T, :]
        out.update(ff=win[..., 0].copy(), oo=win[..., 1].copy(), fo=win[..., 2].copy())
        return self._past(out, n)

    def result(self, sync_dist: bool = False) -> dict:
        cnt = self.counts(sync_dist)
        wb = self.band_w                                                  # [R, H]
        nV = cnt["valid"].astype(np.float64)                              # [L, S, H]
        nF, nO = (cnt[k].astype(np.float64) for k in ("forecast_yes", "observed_yes"))           # [L, S, H, T]
        FF, OO, FO = (cnt[k].astype(np.float64) for k in ("ff", "oo", "fo"))                     # [L, S, H, K, T]
        n2 = (self.window_cells.astype(np.float64) ** 2).T[None, None, :, :, None]               # [1, 1, H, K, 1]
        fold = lambda x: np.einsum("rh,lshkt->lsrkt", wb, x)              # noqa: E731
        fold1 = lambda x: np.einsum("rh,lsht->lsrt", wb, x)               # noqa: E731
        fbs, ref = fold((FF + OO - 2.0 * FO) / n2), fold((FF + OO) / n2)
        sV, sF, sO = np.einsum("rh,lsh->lsr", wb, nV), fold1(nF), fold1(nO)
        base = _ratio(sO, np.broadcast_to(sV[..., None], sO.shape))
        res = {"fss": 1.0 - _ratio(fbs, ref), "fbs": fbs, "fbs_ref": ref, "base_rate": base,
               "frequency_bias": _ratio(sF, sO), "fss_uniform": 0.5 + base / 2.0}
        n = cnt["n_samples"]
        dead = self._dead(n, sF.shape)
        for k in ("base_rate", "frequency_bias", "fss_uniform"):
            res[k] = np.where(dead, np.nan, res[k])
        for k in ("fss", "fbs", "fbs_ref"):
            res[k] = np.where(dead[:, :, :, None, :], np.nan, res[k])
        self._finish(res, n, sV)
        res["scales"] = list(self.scales)
        res["window_cells"] = self.window_cells.copy()
        return res

    skilful_scale = staticmethod(skilful_scale)

    @staticmethod
    def table(result: dict, label: str, band: Optional[str] = None) -> str:
        """plain text, one block per threshold of ``label``: a row per lead, a column per scale (its latitude half-width
        in rows), then ``fss_uniform`` and the index of the skilful scale"""
        s, r, band = lookup(WHO, result, label, band)
        op = ">=" if result["directions"][s] == "ge" else "<="
        first = skilful_scale(result)
        lines = [f"{label} / {band}"]
        for j, t in enumerate(result["thresholds"][s]):
            lines.append(f"{'fss ' + op + format(t, '.4g'):<16}{'count':>8}" +
                         "".join(f"{'ny=' + str(k):>10}" for k in result["scales"]) + f"{'uniform':>10}{'skilful':>9}")
            for lead in range(result["fss"].shape[0]):
                vals = "".join(f"{result['fss'][lead, s, r, k, j]:>10.4f}" for k in range(len(result["scales"])))
                lines.append(f"{lead:<16d}{int(result['count'][lead]):>8d}" + vals +
                             f"{result['fss_uniform'][lead, s, r, j]:>10.4f}{int(first[lead, s, r, j]):>9d}")
            lines.append("")
        return "\n".join(lines[:-1])
