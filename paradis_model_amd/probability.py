"""Probabilistic event verification: when 12 of 16 members forecast the event, does it happen 75 % of the time?  Per lead
time, event source, latitude band and threshold the Brier score (the ensemble's own and the fair one), its
reliability / resolution / uncertainty decomposition, the Brier skill score, the area under the ROC curve and the
curves themselves - reliability diagram, sharpness histogram, ROC points - from integer counts kept on the device.

The definitions are the project's own, textbook formulas; they are NOT pinned against any package.  The tests pin the
kernel against a plain numpy restatement (tests/prob_oracle.py) - exactly: the event decision is discrete and the counts
are integers, so the device result equals the restatement bit for bit, not within a bound.

Conventions.  A forecast state is ``[G * M, C, H, W]`` fp32 in physical units, member-minor: member ``i`` of ensemble
``g`` is batch entry ``g * M + i``, as for ``ensemble.EnsembleCard``.  The truth is ``[G, C, H, W]``: the members of one
ensemble share their truth.  The events are ``events.EventTable``'s, parsed by ``events.parse_events``: a source -
plain channel, ``("speed", a, b)``, ``("anomaly", name)`` - yields one fp32 value ``x`` per cell (``csrc/event_source.h``:
the same bits as in ``EventTable``), the event is ``x >= thr`` (``"ge"``) or ``x <= thr`` (``"le"``), up to
``paradis_events_max_thresholds()`` thresholds per source and ``paradis_events_max_sources()`` sources.  With a
climatology ``[K, C, H, W]``, ``clim_index`` is int32 ``[G]``: one slot per ensemble, since the members share their valid
time.

A cell is valid for a source iff every value it reads is finite: the truth's channel or channels, the climatology cell
of an anomaly, the channel or channels of all ``M`` members.  AN INVALID CELL IS COUNTED NOWHERE (as in ``EventTable``
and ``EnsembleCard``).  An ensemble whose ``clim_index`` is outside ``[0, K)`` has no valid cell for an anomaly source;
nothing of that slot is read.  Per valid cell and threshold ``j``: ``o`` is 1 if the truth has the event, else 0; ``k``
is the number of members that have it, ``0 .. M``; the forecast probability is ``p_k = k / M``.

The device keeps INTEGERS only: per (lead, source, latitude row ``h``) ``nV`` (valid cells) and ``joint[j][o][k]``, the
cells with ``o_j = o`` and ``k_j = k`` - the int64 accumulator ``acc [n_leads, S, H, 1 + T * 2 * (M + 1)]`` (``T``: the
longest threshold list of the table; entries of ``j`` past a source's own list stay 0) and ``n_samples`` int64
``[n_leads]`` (ensembles).  ``sum_{o,k} joint[j][o][k] == nV`` for each of a source's thresholds.  Weights never enter
the kernel: ``result`` applies the band and latitude weights ``wb[r, h]`` to the integer rows on the host, in numpy
float64::

    N_ok = sum_h wb joint[..][o][k]        N_k = N_0k + N_1k        N = sum_k N_k        obar = sum_k N_1k / N

    brier       = sum_k (N_1k (p_k - 1)^2 + N_0k p_k^2) / N
    brier_fair  = brier - sum_k N_k k (M - k) / (M^2 (M - 1) N)       Ferro's estimator, unbiased in M (cf. crps_fair)
    base_rate   = obar                      uncertainty = obar (1 - obar)
    reliability = sum_{k: N_k > 0} N_k (p_k - N_1k / N_k)^2 / N
    resolution  = sum_{k: N_k > 0} N_k (N_1k / N_k - obar)^2 / N
    bss         = 1 - brier / uncertainty
    roc_area    = the trapezoid area under the points (pofd_q, pod_q), q = 0 .. M + 1,
                  pod_q = sum_{k >= q} N_1k / sum_k N_1k,   pofd_q = sum_{k >= q} N_0k / sum_k N_0k

    observed_frequency[k] = N_1k / N_k     forecast_frequency[k] = N_k / N (the sharpness histogram)
    pod[q], pofd[q] for q = 0 .. M

``brier = reliability - resolution + uncertainty`` holds exactly (up to rounding): the bins are the distinct forecast
values.  A zero denominator gives NaN.

One launch pair per ``update`` (``csrc/probability.hip``) reads only the planes of the chosen sources, once:
``4 (M + 1)`` bytes per cell of a plain source, ``8 (M + 1)`` of a speed, ``4 (M + 1) + 4`` of an anomaly.

No CPU fallback: ``update`` needs tensors on the HIP device.  Everything else (argument checks, ``counts``, ``result``,
``table``) works on any device.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._leadtable import check_clim_index, check_member_states, read
from ._tables import dense_state
from .events import EventLeadTable, _ratio, lookup

SCORES = ("brier", "brier_fair", "base_rate", "uncertainty", "reliability", "resolution", "bss", "roc_area")
CURVES = ("observed_frequency", "forecast_frequency", "pod", "pofd")


def max_members() -> int:
    return int(_lib.lib.paradis_prob_max_members())


def bytes_per_cell(kind: int, members: int) -> int:
    """the values one cell of a source reads: the truth and ``members`` members (and the climatology)"""
    return {0: 4 * (members + 1), 1: 8 * (members + 1), 2: 4 * (members + 1) + 4}[int(kind)]


def scores(N0, N1, members: int) -> dict:
    """the eight ``SCORES`` and four ``CURVES`` of weighted joint counts ``N0[..., k]`` (the truth has no event) and
    ``N1[..., k]`` (it has), ``k = 0 .. M`` on the last axis, float64; a zero denominator gives NaN, without warnings.
    Host only."""
    N0, N1 = np.asarray(N0, np.float64), np.asarray(N1, np.float64)
    M = int(members)
    k = np.arange(M + 1, dtype=np.float64)
    p = k / M
    with np.errstate(all="ignore"):
        Nk = N0 + N1
        # sums over k >= q, q = 0 .. M (the whole sums n1, n0 are their first entries: pod[0] = pofd[0] = 1 exactly)
        c1, c0 = np.cumsum(N1[..., ::-1], axis=-1)[..., ::-1], np.cumsum(N0[..., ::-1], axis=-1)[..., ::-1]
        n1, n0 = c1[..., 0], c0[..., 0]
        N = n0 + n1
        obar = _ratio(n1, N)
        brier = _ratio((N1 * (p - 1.0) ** 2 + N0 * p ** 2).sum(axis=-1), N)
        fair = brier - _ratio((Nk * k * (M - k)).sum(axis=-1), float(M * M * (M - 1)) * N)
        ok = _ratio(N1, Nk)                                               # NaN in an empty bin
        some = Nk > 0
        rel = _ratio(np.where(some, Nk * (p - np.where(some, ok, 0.0)) ** 2, 0.0).sum(axis=-1), N)
        res = _ratio(np.where(some, Nk * (np.where(some, ok, 0.0) - obar[..., None]) ** 2, 0.0).sum(axis=-1), N)
        unc = obar * (1.0 - obar)
        # pod[q] = sum_{k >= q} N1 / n1, q = 0 .. M; the curve ends in (0, 0) at q = M + 1
        pod, pofd = _ratio(c1, n1[..., None]), _ratio(c0, n0[..., None])
        zero = np.zeros(pod.shape[:-1] + (1,))
        y, x = np.concatenate([pod, zero], axis=-1), np.concatenate([pofd, zero], axis=-1)
        roc = ((x[..., :-1] - x[..., 1:]) * (y[..., :-1] + y[..., 1:]) * 0.5).sum(axis=-1)
        return {"brier": brier, "brier_fair": fair, "base_rate": obar, "uncertainty": unc, "reliability": rel,
                "resolution": res, "bss": 1.0 - _ratio(brier, unc), "roc_area": roc, "observed_frequency": ok,
                "forecast_frequency": _ratio(Nk, N[..., None]), "pod": pod, "pofd": pofd}


class ProbabilityTable(EventLeadTable):
    """Per-lead joint counts of (truth event, members with the event) of a rollout whose batch is ``G`` ensembles of
    ``members`` members, accumulated on the device, and the probabilistic scores that come from them (module docstring
    for the definitions; the project's own, not pinned against any package; invalid - non-finite - cells are counted
    nowhere).

    ``names``, ``lat_deg``, ``events``, ``bands``, ``weights`` and ``climatology`` as in ``events.EventTable``;
    ``members``: ``M``, 2 .. ``paradis_prob_max_members()`` (32, as ``EnsembleCard``).

    ``acc`` is the int64 ``[n_leads, S, H, 1 + T * 2 * (M + 1)]`` accumulator on ``device`` - ``{nV, joint[T][2][M + 1]}``
    per row, ``T`` the longest threshold list -, ``8 * n_leads * S * H * (1 + 2 T (M + 1))`` bytes: 190 MB at 40 leads, 6
    sources, 721 rows, ``T = 4`` and ``M = 16``; a few KB per lead at 32 x 64.  ``n_samples`` is int64 ``[n_leads]``
    (ensembles seen).

    ``update(lead, forecast, truth, clim_index=None)``: one launch pair on the current stream, no host synchronisation,
    graph-capturable, neither input is written; ``forecast`` ``[G * M, C, H, W]`` and ``truth`` ``[G, C, H, W]`` fp32
    with dense ``[C, H, W]`` states and any batch stride (``chunk[:, slot]`` and ``truth[::M, k]`` are consumed in
    place); ``clim_index`` ``[G]`` int32 on the device (optional with a one-slot climatology).
    ``counts(sync_dist=False)``: one device read (after ONE all-reduce of the int64 accumulators with ``sync_dist``); the
    raw integers ``valid [n_leads, S, H]``, ``joint [n_leads, S, H, T, 2, M + 1]`` (-1 past a source's own thresholds)
    and ``n_samples [n_leads]``.  ``result(sync_dist=False)``: float64, the eight ``SCORES`` ``[n_leads, S, R, T]`` and
    the four ``CURVES`` ``[n_leads, S, R, T, M + 1]`` (NaN past a source's thresholds, for leads never updated and
    wherever a denominator is zero), ``valid_fraction [n_leads, S, R]``, ``count [n_leads]``, ``labels``,
    ``thresholds``, ``directions``, ``bands`` and ``members``.  ``scores(N0, N1, members)``: host only, weighted joint
    counts -> scores and curves.  ``table(result, label, band=, threshold=)``: plain text for logs.  ``reset()`` clears
    the accumulators."""

    NOUN = "the probability table"
    HAS = "the probability table has"
    NEEDS = "a probability table needs"

    def __init__(self, names: Sequence[str], lat_deg, n_leads: int, events: dict, members: int, *,
                 bands: Optional[dict] = None, weights=None, climatology: Optional[torch.Tensor] = None, device="cuda"):
        if isinstance(members, bool) or not isinstance(members, (int, np.integer)) or \
                not 2 <= int(members) <= max_members():
            raise ValueError(f"{type(self).__name__}: members must be an integer in [2, {max_members()}], "
                             f"got {members!r}")
        self.members = int(members)
        super().__init__(names, lat_deg, n_leads, events, bands, weights, climatology, device,
                         row=lambda tmax: 1 + self.T * 2 * (self.members + 1))      # (parse_events has set T by then)
        self._bytes_per_cell = float(sum(bytes_per_cell(k, self.members) for k in self.kinds))

    def _check(self, lead, forecast, truth, clim_index=None, n_lon=None):
        """argument checks of ``update``; returns (G, C, H, W)"""
        G, W = check_member_states(self.who, self.IT_HAS, self.n_leads, self.C, self.H, self.members, lead, forecast,
                                   truth)
        self._check_longitudes(W)
        dense_state(forecast, "forecast", f"{self.who}.update")
        dense_state(truth, "truth", f"{self.who}.update")
        check_clim_index(self.who, self.IT_HAS, self.climatology, clim_index, G, W)
        return G, self.C, self.H, W

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor,
               clim_index: Optional[torch.Tensor] = None) -> None:
        G, C, H, W = self._check(lead, forecast, truth, clim_index)
        M, T, S = self.members, self.T, len(self.labels)
        self._launch("prob_update", _lib.lib.paradis_prob_ws_bytes(G, S, H, W, M, T), lead, forecast, truth, clim_index, G,
                     G, M, T, C, S, H, W)

    def _joint(self, sync_dist: bool):
        """one device read: ``(nV [L, S, H], joint [L, S, H, T, 2, M + 1], n_samples)``"""
        a, n = read(self.acc, self.n_samples, sync_dist)
        joint = a[..., 1:].reshape(a.shape[:3] + (self.T, 2, self.members + 1))
        return a[..., 0].copy(), joint.copy(), n

    def counts(self, sync_dist: bool = False) -> dict:
        nV, joint, n = self._joint(sync_dist)
        for s, nt in enumerate(self.n_thresholds):
            joint[:, s, :, nt:] = -1
        return {"valid": nV, "joint": joint, "n_samples": n}

    def result(self, sync_dist: bool = False) -> dict:
        nV, joint, n = self._joint(sync_dist)
        wb = self.band_w                                                  # [R, H]
        Nok = np.einsum("rh,lshtok->lsrtok", wb, joint.astype(np.float64))
        res = scores(Nok[..., 0, :], Nok[..., 1, :], self.members)
        dead = self._dead(n, Nok.shape[:4])
        for k in SCORES:
            res[k] = np.where(dead, np.nan, res[k])
        for k in CURVES:
            res[k] = np.where(dead[..., None], np.nan, res[k])
        res["members"] = self.members
        return self._finish(res, n, np.einsum("rh,lsh->lsr", wb, nV.astype(np.float64)))

    scores = staticmethod(scores)

    @staticmethod
    def table(result: dict, label: str, band: Optional[str] = None, threshold: int = 0) -> str:
        """plain text: a row per lead with ``count`` and the eight ``SCORES`` of threshold number ``threshold`` of
        ``label``, then its reliability diagram - per lead a row of ``forecast_frequency`` and a row of
        ``observed_frequency`` over the forecast probabilities ``k / M``"""
        s, r, band = lookup("ProbabilityTable", result, label, band)
        thr = result["thresholds"][s]
        if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or \
                not 0 <= int(threshold) < len(thr):
            raise ValueError(f"ProbabilityTable.table: threshold must be an index in [0, {len(thr)}) of event "
                             f"'{label}', got {threshold!r}")
        j, M = int(threshold), int(result["members"])
        op = ">=" if result["directions"][s] == "ge" else "<="
        lines = [f"{label} {op} {thr[j]:.4g} / {band} / {M} members"]
        lines.append(f"{'lead':<6}{'count':>8}" + "".join(f"{m:>13}" for m in SCORES))
        n_leads = len(result["count"])
        for lead in range(n_leads):
            vals = "".join(f"{result[m][lead, s, r, j]:>13.5g}" for m in SCORES)
            lines.append(f"{lead:<6d}{int(result['count'][lead]):>8d}" + vals)
        lines.append("")
        lines.append(f"{'lead':<6}{'p = k / M':>10}" + "".join(f"{k / M:>8.3f}" for k in range(M + 1)))
        for lead in range(n_leads):
            for name, key in (("forecast", "forecast_frequency"), ("observed", "observed_frequency")):
                vals = "".join(f"{result[key][lead, s, r, j, k]:>8.4f}" for k in range(M + 1))
                lines.append(f"{lead:<6d}{name:>10}" + vals)
        return "\n".join(lines)
