"""Event verification: did the forecast put the event where it happened?  Per lead time, event source, latitude band and
threshold the 2x2 contingency table of "value beyond a threshold" in forecast against truth, counted on the device in
integers, and the categorical scores that come from it (POD, FAR, POFD, CSI, frequency bias, base rate, ETS, HSS, SEDI).

The definitions are the project's own, textbook formulas; they are NOT pinned against any package.  The tests pin the
kernel against a plain numpy restatement (tests/events_oracle.py) - exactly: the event decision is discrete and the
counts are integers, so the device result equals the restatement bit for bit, not within a bound.

Conventions.  Forecast ``f`` and truth ``t`` are ``[B, C, H, W]`` fp32 in physical units, in the chunk layout of
``forecast.postprocess`` (``PostSpec.names``).  An event source yields one fp32 value ``x`` per cell::

    "name"                        plain     x = v[c]
    ("speed", "name_a", "name_b") speed     x = sqrtf(a*a + b*b)             (fp32: mul, mul, add, sqrt, uncontracted)
    ("anomaly", "name")           anomaly   x = v[c] - clim[k[b]][c]         (one fp32 subtraction)

with 1 to ``paradis_events_max_thresholds()`` thresholds in physical units (rounded to fp32; they need not be sorted)
and a direction: ``"ge"`` (event: ``x >= thr``) or ``"le"`` (``x <= thr``; handed to the kernel as ``sign = -1``,
``thr' = -thr``, which is exact).  ``x == thr`` is an event in both directions, ``-0.0 >= 0.0`` is one.

A cell is valid for a source iff every input value it reads is finite: forecast and truth, both components of a speed
source, the climatology cell of an anomaly source.  A sample whose ``clim_index`` is outside ``[0, K)`` has no valid cell
for anomaly sources (nothing of that slot is read).  INVALID CELLS ARE COUNTED IN NO CLASS.  This departs from
``verify.Scorecard`` and ``spectrum.Spectra``, where non-finite values propagate into the scores: a count cannot carry a
NaN.  ``valid_fraction`` reports how much was counted.

Per valid cell and threshold ``j``, ``F``: the forecast is beyond the threshold, ``O``: the truth is.  The device keeps,
per (lead, source, latitude row ``h``), ``nV`` (valid cells) and ``nF[j]``, ``nO[j]``, ``nFO[j]``: the int64 accumulator
``acc [n_leads, S, H, 1 + 3 * TMAX]`` and ``n_samples`` int64 ``[n_leads]``.  Weights never enter the kernel:
``result`` applies the band and latitude weights ``wb[r, h]`` to the integer rows on the host, in numpy float64::

    hits a = sum_h wb nFO      false alarms b = sum_h wb (nF - nFO)      misses c = sum_h wb (nO - nFO)
    correct negatives d = sum_h wb (nV - nF - nO + nFO)                  n = a + b + c + d

    pod = a/(a+c)   far = b/(a+b)   pofd = b/(b+d)   csi = a/(a+b+c)   frequency_bias = (a+b)/(a+c)   base_rate = (a+c)/n
    ets = (a - ar)/(a+b+c - ar),  ar = (a+b)(a+c)/n          hss = 2(ad - bc)/((a+c)(c+d) + (a+b)(b+d))
    sedi = (ln pofd - ln pod - ln(1-pofd) + ln(1-pod)) / (ln pofd + ln pod + ln(1-pofd) + ln(1-pod))

A zero denominator or a ``ln 0`` gives NaN.

One launch pair per ``update`` (``csrc/events.hip``) reads only the planes of the chosen sources, once.

No CPU fallback: ``update`` needs tensors on the HIP device.  Everything else (argument checks, ``counts``, ``result``,
``scores``, ``table``) works on any device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr
from ._leadtable import LeadTable, positive_int, read, resolve_clim_index
from ._tables import batch_stride, workspace

KINDS = {"plain": 0, "speed": 1, "anomaly": 2}
BYTES_PER_CELL = {0: 8, 1: 16, 2: 12}          # forecast and truth (and climatology) values of one cell
TABLES = ("hits", "false_alarms", "misses", "correct_negatives")
SCORES = ("pod", "far", "pofd", "csi", "frequency_bias", "base_rate", "ets", "hss", "sedi")


def max_thresholds() -> int:
    return int(_lib.lib.paradis_events_max_thresholds())


def _ratio(num, den):
    """``num / den``, NaN where ``den == 0``"""
    ok = den != 0
    return np.where(ok, num / np.where(ok, den, 1.0), np.nan)


def _ln(x):
    """``ln x``, NaN where ``x <= 0`` (a ``ln 0`` is NaN here, not -inf)"""
    ok = x > 0
    return np.where(ok, np.log(np.where(ok, x, 1.0)), np.nan)


def scores(a, b, c, d) -> dict:
    """the nine scores of 2x2 tables (hits ``a``, false alarms ``b``, misses ``c``, correct negatives ``d``: arrays of one
    shape, or numbers), float64; a zero denominator or a ``ln 0`` gives NaN, without warnings.  Host only."""
    a, b, c, d = (np.asarray(v, np.float64) for v in (a, b, c, d))
    with np.errstate(all="ignore"):
        n = a + b + c + d
        pod, pofd = _ratio(a, a + c), _ratio(b, b + d)
        ar = _ratio((a + b) * (a + c), n)
        lf, lh, l1f, l1h = _ln(pofd), _ln(pod), _ln(1.0 - pofd), _ln(1.0 - pod)
        return {"pod": pod, "far": _ratio(b, a + b), "pofd": pofd, "csi": _ratio(a, a + b + c),
                "frequency_bias": _ratio(a + b, a + c), "base_rate": _ratio(a + c, n),
                "ets": _ratio(a - ar, a + b + c - ar),
                "hss": _ratio(2.0 * (a * d - b * c), (a + c) * (c + d) + (a + b) * (b + d)),
                "sedi": _ratio(lf - lh - l1f + l1h, lf + lh + l1f + l1h)}


def parse_events(who: str, events, names: Sequence[str], with_climatology: bool) -> dict:
    """the ``events`` dict of ``EventTable`` (and ``neighbourhood.FractionsTable``) checked and turned into the attributes
    both keep: ``tmax``, ``labels``, ``thresholds``, ``directions``, ``kinds``, ``n_thresholds``, ``T`` and the two host
    tables of the entry points, ``_src`` int32 ``[S, 4]`` and ``_thr`` float32 ``[S, 1 + tmax]``, and
    ``_bytes_per_cell``.  ``who`` opens every message."""
    names = list(names)

    def channel(label, name) -> int:
        if not isinstance(name, str) or name not in names:
            raise ValueError(f"{who}: event '{label}': channel {name!r} is not among the names")
        return names.index(name)

    tmax = max_thresholds()
    smax = int(_lib.lib.paradis_events_max_sources())
    if not isinstance(events, dict) or len(events) < 1:
        raise ValueError(f"{who}: events must be a non-empty dict label -> {{source, thresholds, direction}}")
    if len(events) > smax:
        raise ValueError(f"{who}: {len(events)} events, at most {smax} go into one table")
    labels: List[str] = []
    thresholds: List[List[float]] = []
    directions: List[str] = []
    src = np.zeros((len(events), 4), np.int32)
    thr = np.zeros((len(events), 1 + tmax), np.float32)
    for s, (label, ev) in enumerate(events.items()):
        label = str(label)
        if not isinstance(ev, dict) or "source" not in ev or "thresholds" not in ev or \
                set(ev) - {"source", "thresholds", "direction"}:
            raise ValueError(f"{who}: event '{label}' must be a dict with source, thresholds and, optionally, "
                             f"direction")
        source = ev["source"]
        if isinstance(source, str):
            kind, c0, c1 = KINDS["plain"], channel(label, source), 0
        elif isinstance(source, (tuple, list)) and len(source) == 3 and source[0] == "speed":
            kind, c0, c1 = KINDS["speed"], channel(label, source[1]), channel(label, source[2])
            if c0 == c1:
                raise ValueError(f"{who}: event '{label}': the speed of '{source[1]}' with itself is refused "
                                 f"(take the plain channel with both directions instead)")
        elif isinstance(source, (tuple, list)) and len(source) == 2 and source[0] == "anomaly":
            kind, c0, c1 = KINDS["anomaly"], channel(label, source[1]), 0
            if not with_climatology:
                raise ValueError(f"{who}: event '{label}' is an anomaly, but the table has no climatology")
        else:
            raise ValueError(f"{who}: event '{label}': source must be 'name', ('speed', a, b) or "
                             f"('anomaly', name), got {source!r}")
        direction = ev.get("direction", "ge")
        if direction not in ("ge", "le"):
            raise ValueError(f"{who}: event '{label}': direction must be 'ge' or 'le', got {direction!r}")
        try:
            t64 = np.asarray(list(ev["thresholds"]), np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: event '{label}': thresholds must be a list of numbers") from None
        if not 1 <= t64.size <= tmax:
            raise ValueError(f"{who}: event '{label}' has {t64.size} thresholds, 1 to {tmax} are allowed")
        with np.errstate(over="ignore"):
            t32 = t64.astype(np.float32)
        if not np.isfinite(t64).all() or not np.isfinite(t32).all():
            raise ValueError(f"{who}: event '{label}': thresholds must be finite (in float32)")
        sign = np.float32(1.0 if direction == "ge" else -1.0)
        src[s] = (kind, c0, c1, t32.size)
        thr[s, 0] = sign
        thr[s, 1:1 + t32.size] = sign * t32
        labels.append(label)
        thresholds.append([float(v) for v in t32])
        directions.append(direction)
    kinds = [int(k) for k in src[:, 0]]
    n_thresholds = [int(n) for n in src[:, 3]]
    return {"tmax": tmax, "labels": labels, "thresholds": thresholds, "directions": directions, "kinds": kinds,
            "n_thresholds": n_thresholds, "T": max(n_thresholds), "_src": np.ascontiguousarray(src),
            "_thr": np.ascontiguousarray(thr), "_bytes_per_cell": float(sum(BYTES_PER_CELL[k] for k in kinds))}


class EventLeadTable(LeadTable):
    """What ``EventTable`` and ``neighbourhood.FractionsTable`` share: construction up to ``parse_events``, the int64
    accumulator rows that begin ``{nV, nF[TMAX], nO[TMAX]}`` and ``n_samples``, the parts of ``counts`` / ``result``
    that read them, ``bind`` and the one path of ``update`` into an entry point (``_launch``).  ``n_lon``: the number of
    longitudes where the constructor knows it; ``row``: the int64 entries of one accumulator row, given ``tmax``.
    ``probability.ProbabilityTable`` sits on it too, with rows of its own (``{nV, joint[T][2][M + 1]}``): it takes the
    construction, ``reset``, ``bind``, ``_launch``, ``_dead`` and ``_finish`` and leaves ``_counts_head`` / ``_past``
    alone."""
    IT = "the table"
    IT_HAS = "the table has"

    def __init__(self, names, lat_deg, n_leads, events, bands, weights, climatology, device, row, n_lon=None):
        super().__init__(names, n_leads, device)
        if n_lon is not None:
            self.W = positive_int(self.who, "n_lon", n_lon)
        self.lat = self._set_grid(lat_deg, weights, bands)
        self._set_climatology(climatology)
        for k, v in parse_events(self.who, events, self.names, self.climatology is not None).items():
            setattr(self, k, v)
        with torch.inference_mode(False):
            self.acc = torch.zeros(self.n_leads, len(self.labels), self.H, row(self.tmax), dtype=torch.int64,
                                   device=self.device)
            self.n_samples = torch.zeros(self.n_leads, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.acc.zero_()
        self.n_samples.zero_()

    def bind(self, W: int) -> None:
        """states the number of longitudes ahead of the first ``update`` (which otherwise does it); ``valid_fraction``
        needs it"""
        W = positive_int(f"{self.who}.bind", "W", W)
        if self.W is not None and W != self.W:
            raise ValueError(f"{self.who}.bind: the table is bound to {self.W} longitudes already")
        self.W = W

    def _check_longitudes(self, W: int) -> None:
        if self.W is not None and W != self.W:
            raise ValueError(f"{self.who}.update: forecast has {W} longitudes, the table is bound to {self.W}")

    def _entry_tables(self, device) -> tuple:
        """the tables an entry point takes behind ``thr_table`` (``FractionsTable``: its half-widths)"""
        return ()

    def _launch(self, entry: str, ws_bytes: int, lead, forecast, truth, clim_index, n: int, *tail) -> None:
        """what ``update`` does once its table has checked the arguments: ``entry`` on the current stream for ``n``
        samples (ensembles), with the arguments every event entry point begins with, then the shape ``tail``;
        ``ws_bytes``: what the entry point's ``*_ws_bytes`` asks for"""
        require_hip(forecast, truth)
        if not self.acc.is_cuda:
            raise RuntimeError(f"{self.who}.update: the table was made with a CPU device (there is no CPU fallback)")
        if n == 0:             # (empty tensors have no address to hand over; the entry point would do nothing either)
            return
        C, H, W = forecast.shape[1:]
        if self.W is None:
            self.bind(W)
        clim = self.climatology
        clim_index = resolve_clim_index(self.who, self._slot0, clim, clim_index, n, forecast.device)
        tables = self._entry_tables(forecast.device)          # (in front of the workspace, as FractionsTable had it)
        ws = workspace(self._ws, forecast.device, int(ws_bytes))
        _lib.call(entry, self._bytes_per_cell * n * H * W, dptr(forecast), batch_stride(forecast, C * H * W),
                  dptr(truth), batch_stride(truth, C * H * W), dptr(clim), dptr(clim_index),
                  0 if clim_index is None else clim.shape[0], self._src.ctypes.data, self._thr.ctypes.data, *tables,
                  dptr(self.acc[int(lead)]), dptr(self.n_samples[int(lead):]), dptr(ws), *tail, stream_ptr())

    def _counts_head(self, sync_dist: bool):
        """one device read: ``(a, n_samples, out)`` - the accumulator, the sample counts and ``out`` with ``valid``,
        ``forecast_yes`` and ``observed_yes``; ``_past`` marks what a subclass adds"""
        a, n = read(self.acc, self.n_samples, sync_dist)
        T, TM = self.T, self.tmax
        out = {"valid": a[..., 0].copy(), "forecast_yes": a[..., 1:1 + T].copy(),
               "observed_yes": a[..., 1 + TM:1 + TM + T].copy()}
        return a, n, out

    def _past(self, out: dict, n) -> dict:
        """-1 past a source's own thresholds (the last axis of every array but ``valid``), then ``n_samples``"""
        for s, nt in enumerate(self.n_thresholds):
            for k in out:
                if k != "valid":
                    out[k][:, s, ..., nt:] = -1
        out["n_samples"] = n
        return out

    def _dead(self, n, shape) -> np.ndarray:
        """bool ``[n_leads, S, R, T]``: leads never updated, and entries past a source's own thresholds"""
        dead = np.zeros(shape, bool)
        dead[n == 0] = True
        for s, nt in enumerate(self.n_thresholds):
            dead[:, s, :, nt:] = True
        return dead

    def _finish(self, res: dict, n, sV) -> dict:
        """``valid_fraction`` from ``sV = sum_h wb nV`` ``[n_leads, S, R]``, and what every result ends with"""
        seen = n.astype(np.float64)[:, None, None] * float(self.W or 0) * self.band_w.sum(axis=1)[None, None, :]
        with np.errstate(all="ignore"):
            res["valid_fraction"] = sV / np.where(seen > 0, seen, np.nan)
        res["count"] = n.copy()
        res["labels"] = list(self.labels)
        res["thresholds"] = [list(t) for t in self.thresholds]
        res["directions"] = list(self.directions)
        res["bands"] = list(self.bands)
        return res


def lookup(who: str, result: dict, label: str, band: Optional[str]):
    """``(s, r, band)``: where ``label`` and ``band`` (default the first) are in a result, for ``table``"""
    labels: List[str] = list(result["labels"])
    bands: List[str] = list(result["bands"])
    if str(label) not in labels:
        raise ValueError(f"{who}.table: event '{label}' is not among the table's labels")
    band = bands[0] if band is None else str(band)
    if band not in bands:
        raise ValueError(f"{who}.table: band '{band}' is not among the table's bands")
    return labels.index(str(label)), bands.index(band), band


class EventTable(EventLeadTable):
    """Per-lead contingency tables of threshold events, accumulated on the device (module docstring for the definitions;
    invalid - non-finite - cells are counted in no class, unlike ``Scorecard``, where NaN propagates).

    ``names``: the chunk's channel names (``PostSpec.names``); ``lat_deg``: ``[H]`` latitudes in degrees; ``events``: a
    dict label -> ``{"source": "name" | ("speed", a, b) | ("anomaly", name), "thresholds": [1 .. TMAX finite numbers],
    "direction": "ge" | "le"}`` (direction defaults to ``"ge"``), at most ``paradis_events_max_sources()`` entries; a
    speed of one channel with itself is refused.  ``bands`` and ``weights`` as in ``spectrum.Spectra``: a dict name ->
    ``(lat_lo, lat_hi)`` in degrees, inclusive (default ``{"global": (-90, 90)}``), row weights ``weights[h]`` inside a
    band and 0 outside (default ``cos(lat)``, pole rows 0).  ``climatology``: ``[K, C, H, W]`` fp32 on the device, as in
    ``Scorecard``; anomaly sources need one.

    ``acc`` is the int64 ``[n_leads, S, H, 1 + 3 * TMAX]`` accumulator on ``device`` - ``{nV, nF[TMAX], nO[TMAX],
    nFO[TMAX]}`` per row -, ``n_leads * S * H * 200`` bytes: 35 MB at 721 rows, 6 sources and 40 leads, a few KB per lead
    at 32 x 64.  ``n_samples`` is int64 ``[n_leads]``.

    ``update(lead, forecast, truth, clim_index=None)``: one launch pair on the current stream, no host synchronisation,
    graph-capturable, neither input is written; ``forecast`` / ``truth`` ``[B, C, H, W]`` fp32 with dense ``[C, H, W]``
    states and any batch stride; ``clim_index`` ``[B]`` int32 on the device (optional with a one-slot climatology).
    ``counts(sync_dist=False)``: one device read (after ONE all-reduce of the int64 accumulators with ``sync_dist``);
    the raw integers ``valid [n_leads, S, H]``, ``forecast_yes``, ``observed_yes``, ``both [n_leads, S, H, T]`` (``T``:
    the longest threshold list; entries past a source's own list are -1) and ``n_samples [n_leads]``.
    ``result(sync_dist=False)``: float64 ``hits``, ``false_alarms``, ``misses``, ``correct_negatives`` and the nine
    ``SCORES``, each ``[n_leads, S, R, T]`` (NaN past a source's thresholds and for leads never updated),
    ``valid_fraction [n_leads, S, R]`` (the weighted share of the cells seen that were valid), ``count [n_leads]``,
    ``labels``, ``thresholds`` (per label, as given, after rounding to fp32), ``directions`` and ``bands``.
    ``scores(a, b, c, d)``: host only, tables -> the nine scores.  ``table(result, label, ...)``: plain text for logs.
    ``reset()`` clears the accumulators."""

    NOUN = "the event table"
    HAS = "the event table has"
    NEEDS = "an event table needs"

    def __init__(self, names: Sequence[str], lat_deg, n_leads: int, events: dict, *, bands: Optional[dict] = None,
                 weights=None, climatology: Optional[torch.Tensor] = None, device="cuda"):
        super().__init__(names, lat_deg, n_leads, events, bands, weights, climatology, device,
                         row=lambda tmax: 1 + 3 * tmax)

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor,
               clim_index: Optional[torch.Tensor] = None) -> None:
        B, C, H, W = self._check(lead, forecast, truth, clim_index)
        S = len(self.labels)
        self._launch("events_update", _lib.lib.paradis_events_ws_bytes(B, S, H, W), lead, forecast, truth, clim_index, B,
                     B, C, S, H, W)

    def counts(self, sync_dist: bool = False) -> dict:
        a, n, out = self._counts_head(sync_dist)
        out["both"] = a[..., 1 + 2 * self.tmax:1 + 2 * self.tmax + self.T].copy()
        return self._past(out, n)

    def result(self, sync_dist: bool = False) -> dict:
        cnt = self.counts(sync_dist)
        wb = self.band_w                                                  # [R, H]
        nV = cnt["valid"].astype(np.float64)                              # [L, S, H]
        nF, nO, nFO = (cnt[k].astype(np.float64) for k in ("forecast_yes", "observed_yes", "both"))   # [L, S, H, T]
        fold = lambda x: np.einsum("rh,lsht->lsrt", wb, x)                # noqa: E731
        a, b, c = fold(nFO), fold(nF - nFO), fold(nO - nFO)
        d = fold(nV[..., None] - nF - nO + nFO)
        res = dict(zip(TABLES, (a, b, c, d)))
        res.update(scores(a, b, c, d))
        n = cnt["n_samples"]
        dead = self._dead(n, a.shape)
        for k in TABLES + SCORES:
            res[k] = np.where(dead, np.nan, res[k])
        return self._finish(res, n, np.einsum("rh,lsh->lsr", wb, nV))

    scores = staticmethod(scores)

    @staticmethod
    def table(result: dict, label: str, band: Optional[str] = None,
              metrics: Sequence[str] = ("frequency_bias", "csi", "ets", "sedi")) -> str:
        """plain text, one block per metric: a row per lead, a column per threshold of ``label``"""
        s, r, band = lookup("EventTable", result, label, band)
        for m in metrics:
            if m not in TABLES + SCORES:
                raise ValueError(f"EventTable.table: '{m}' is not among {TABLES + SCORES}")
        thr = result["thresholds"][s]
        op = ">=" if result["directions"][s] == "ge" else "<="
        lines = [f"{label} / {band}"]
        for m in metrics:
            lines.append(f"{m:<16}{'count':>8}" + "".join(f"{op + format(t, '.4g'):>12}" for t in thr))
            for lead in range(result[m].shape[0]):
                vals = "".join(f"{result[m][lead, s, r, j]:>12.4f}" for j in range(len(thr)))
                lines.append(f"{lead:<16d}{int(result['count'][lead]):>8d}" + vals)
            lines.append("")
        return "\n".join(lines[:-1])
