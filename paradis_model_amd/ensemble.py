"""Ensemble verification: is the ensemble sharp, and does its spread say how wrong it is?  Per lead time, channel and
latitude band the CRPS (the ensemble's own and the fair one), the RMSE of the ensemble mean, the spread, their ratio and
the rank histogram of the truth among the members, accumulated on the device.

The definitions are the project's own, textbook formulas in the spirit of WeatherBench-2's probabilistic metrics; they
are NOT pinned against any package.  The tests pin the kernel against a plain numpy restatement (tests/ens_oracle.py):
the integers (valid cells, rank histogram) bit for bit, the double row sums within the rounding of a reordered double
sum of the same fp32 terms.

Conventions.  A forecast state is ``[G * M, C, H, W]`` fp32 in physical units, member-minor: member ``i`` of ensemble
``g`` is batch entry ``g * M + i`` (a ``Forecaster.run`` batch of ``B = G * M`` perturbed or lagged initial states).
The truth is ``[G, C, H, W]``: the members of one ensemble share their truth.  A cell is valid iff its truth ``y`` and
all ``M`` member values ``x_i`` are finite; AN INVALID CELL ADDS NOTHING ANYWHERE (as in ``events.EventTable``: a count
cannot carry a NaN).  Per valid cell, all in fp32, uncontracted, in exactly this order (``rM = float32(1) / float32(M)``)::

    A  = sum_i |x_i - y|                      i = 0 .. M-1 ascending, starting from 0.0f
    P  = sum_{i<j} |x_i - x_j|                i ascending, then j ascending
    m  = (sum_i x_i) * rM                     the ensemble mean
    E2 = (m - y) * (m - y)
    V  = sum_i (x_i - m) * (x_i - m)
    lo = #{i : x_i < y}      eq = #{i : x_i == y}
    r  = lo + hash32(key) % (eq + 1)          the truth's rank in 0 .. M, ties broken by a fixed hash
    key = uint32(((n * C + c) * H + h) * W + w) + uint32(salt) * 0x9E3779B9        (all mod 2^32)
    hash32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16

``c`` is the channel's index in the state (not in a ``channels=`` subset), ``n`` the ordinal of the ensemble at this
lead - the lead's ``n_samples`` before this update plus ``g``, so that two updates break ties exactly as one update of
the concatenated ensembles - and ``salt = seed + lead``.  No sort: ``P`` is the spread term of the CRPS, ``lo`` / ``eq``
give the rank.

The device keeps, per (lead, chosen channel, latitude row ``h``), the doubles ``{sum A, sum P, sum E2, sum V}`` (each
cell term widened to double before it meets another cell's) and the integers ``{nV, hist[0 .. M]}``, and ``n_samples``
per lead.  Weights never enter the kernel: ``result`` applies the band and latitude weights ``wb[r, h]`` on the host, in
numpy float64.  With ``N = sum_h wb nV`` and ``S_X = sum_h wb X``::

    mae_members  = S_A / (M N)
    crps         = S_A / (M N) - S_P / (M^2 N)           the ensemble's own CDF
    crps_fair    = S_A / (M N) - S_P / (M (M-1) N)       unbiased in M; the one WeatherBench-2 reports
    rmse_mean    = sqrt(S_E2 / N)
    spread       = sqrt(S_V / ((M-1) N))
    spread_skill = sqrt((M+1) / M) * spread / rmse_mean
    rank_hist[r] = S_hist[r] / N                         (sums to 1)
    outliers     = rank_hist[0] + rank_hist[M]

One launch pair per ``update`` (``csrc/ensemble.hip``) reads only the planes of the chosen channels, once.

No CPU fallback: ``update`` needs tensors on the HIP device.  Everything else (argument checks, ``counts``, ``result``,
``table``) works on any device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr
from ._leadtable import LeadTable, check_member_states, read
from ._tables import batch_stride, dense_state, workspace

REAL_FIELDS = 4          # {sum A, sum P, sum E2, sum V}
METRICS = ("mae_members", "crps", "crps_fair", "rmse_mean", "spread", "spread_skill", "outliers")


def max_members() -> int:
    return int(_lib.lib.paradis_ens_max_members())


def report(real: np.ndarray, ints: np.ndarray, n: np.ndarray, band_w: np.ndarray, members: int, names, bands) -> dict:
    """``real`` double ``[n_leads, Cs, H, 4]``, ``ints`` int64 ``[n_leads, Cs, H, 2 + M]``, ``n`` ``[n_leads]`` and the
    band weights ``[R, H]`` -> the reported values (``EnsembleCard.result``).  Host only."""
    M = float(members)
    wb = np.asarray(band_w, np.float64)
    N = np.einsum("rh,lch->lcr", wb, ints[..., 0].astype(np.float64))
    S = np.einsum("rh,lchk->lcrk", wb, np.asarray(real, np.float64))
    hist = np.einsum("rh,lchk->lcrk", wb, ints[..., 1:].astype(np.float64))
    dead = (np.asarray(n).reshape(-1, 1, 1) == 0) | (N == 0)
    with np.errstate(all="ignore"):
        Nn = np.where(dead, np.nan, N)
        mae = S[..., 0] / (M * Nn)
        res = {"mae_members": mae, "crps": mae - S[..., 1] / (M * M * Nn),
               "crps_fair": mae - S[..., 1] / (M * (M - 1.0) * Nn), "rmse_mean": np.sqrt(S[..., 2] / Nn),
               "spread": np.sqrt(S[..., 3] / ((M - 1.0) * Nn))}
        res["spread_skill"] = np.sqrt((M + 1.0) / M) * res["spread"] / res["rmse_mean"]
        res["rank_hist"] = hist / Nn[..., None]
        res["outliers"] = res["rank_hist"][..., 0] + res["rank_hist"][..., -1]
    res["count"] = np.asarray(n).copy()
    res["names"] = list(names)
    res["bands"] = list(bands)
    res["members"] = int(members)
    return res


class EnsembleCard(LeadTable):
    """Per-lead ensemble scores of a rollout whose batch is ``G`` ensembles of ``members`` members, accumulated on the
    device (module docstring for the formulas; the project's own definitions, not pinned against any package; invalid -
    non-finite - cells add nothing, unlike ``Scorecard``, where NaN propagates).

    ``names``: the chunk's channel names (``PostSpec.names``); ``lat_deg``: ``[H]`` latitudes in degrees; ``members``:
    ``M``, 2 .. ``paradis_ens_max_members()``; ``bands`` and ``weights`` as in ``spectrum.Spectra``: a dict name ->
    ``(lat_lo, lat_hi)`` in degrees, inclusive (default ``{"global": (-90, 90)}``), row weights ``weights[h]`` inside a
    band and 0 outside (default ``cos(lat)``, pole rows 0); ``channels``: the subset of ``names`` to score (default
    all), in any order - only these planes are read; ``all_names`` stays the state's names, ``names`` the subset;
    ``seed``: enters the tie-breaking hash of the ranks (``salt = seed + lead``) and nothing else.

    The accumulators live on ``device``: ``acc_real`` double ``[n_leads, Cs, H, 4]``, ``acc_int`` int64 ``[n_leads, Cs,
    H, 2 + M]`` and ``n_samples`` int64 ``[n_leads]`` (ensembles seen) - ``n_leads * Cs * H * (4 + 2 + M)`` 8-byte words:
    about 0.5 GB for 40 leads of 96 channels at 721 rows with M = 16, which is what ``channels=`` is for.

    ``update(lead, forecast, truth)``: one launch pair on the current stream, no host synchronisation, graph-capturable,
    neither input is written; ``forecast`` ``[G * M, C, H, W]`` and ``truth`` ``[G, C, H, W]`` fp32 with dense
    ``[C, H, W]`` states and any batch stride (``chunk[:, slot]`` and ``truth[::M, k]`` are consumed in place).
    ``counts(sync_dist=False)``: the raw accumulators, ``sums [n_leads, Cs, H, 4]`` float64, ``valid [n_leads, Cs, H]``
    and ``rank_counts [n_leads, Cs, H, M + 1]`` int64, ``n_samples [n_leads]``.  ``result(sync_dist=False)``: one device
    read (after ONE all-reduce with ``sync_dist``; the integers travel as doubles, exact below 2^53); the seven
    ``METRICS`` as float64 ``[n_leads, Cs, R]``, ``rank_hist [n_leads, Cs, R, M + 1]``, ``count [n_leads]``, ``names``
    (the chosen channels), ``bands`` and ``members``; leads never updated come back as NaN with count 0.
    ``table(result, channel, band=...)``: plain text for logs.  ``reset()`` clears the accumulators (and with
    ``n_samples`` the ordinal that the tie-breaking counts from)."""

    IT = "the card"
    IT_HAS = "the card has"
    NOUN = "the ensemble card"
    HAS = "the ensemble card has"
    NEEDS = "an ensemble card needs"
    TAKES_CLIM_INDEX = False

    def __init__(self, names: Sequence[str], lat_deg, n_leads: int, members: int, *, bands: Optional[dict] = None,
                 weights=None, channels: Optional[Sequence[str]] = None, seed: int = 0, device="cuda"):
        super().__init__(names, n_leads, device)
        self._set_grid(lat_deg, weights, bands)
        if isinstance(members, bool) or not isinstance(members, (int, np.integer)) or \
                not 2 <= int(members) <= max_members():
            raise ValueError(f"EnsembleCard: members must be an integer in [2, {max_members()}], got {members!r}")
        self.members = int(members)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
            raise ValueError(f"EnsembleCard: seed must be an integer >= 0, got {seed!r}")
        self.seed = int(seed)
        self._set_channels(channels)
        self._rM = float(np.float32(1.0) / np.float32(self.members))
        Cs = len(self.names)
        with torch.inference_mode(False):
            self._chan = torch.tensor(self.index, dtype=torch.int32, device=self.device)
            self.acc_real = torch.zeros(self.n_leads, Cs, self.H, REAL_FIELDS, dtype=torch.float64, device=self.device)
            self.acc_int = torch.zeros(self.n_leads, Cs, self.H, 2 + self.members, dtype=torch.int64,
                                       device=self.device)
            self.n_samples = torch.zeros(self.n_leads, dtype=torch.int64, device=self.device)

    def _check(self, lead, forecast, truth, clim_index=None, n_lon=None):
        """argument checks of ``update``; returns (G, C, H, W)"""
        G, W = check_member_states(self.who, self.IT_HAS, self.n_leads, self.C, self.H, self.members, lead, forecast,
                                   truth)
        dense_state(forecast, "forecast", f"{self.who}.update")
        dense_state(truth, "truth", f"{self.who}.update")
        return G, self.C, self.H, W

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor) -> None:
        G, C, H, W = self._check(lead, forecast, truth)
        require_hip(forecast, truth)
        if not self.acc_real.is_cuda:
            raise RuntimeError("EnsembleCard.update: the card was made with a CPU device (there is no CPU fallback)")
        if G == 0:             # (empty tensors have no address to hand over; the entry point would do nothing either)
            return
        M, Cs, P = self.members, len(self.names), H * W
        lead = int(lead)
        ws = workspace(self._ws, forecast.device, int(_lib.lib.paradis_ens_ws_bytes(G, Cs, H, W, M)))
        _lib.call("ens_update", 4.0 * (M + 1) * G * Cs * P, dptr(forecast), batch_stride(forecast, C * P), dptr(truth),
                  batch_stride(truth, C * P), dptr(self._chan), self._rM, (self.seed + lead) & 0xFFFFFFFF,
                  dptr(self.acc_real[lead]), dptr(self.acc_int[lead]), dptr(self.n_samples[lead:]), dptr(ws), G, M, C,
                  Cs, H, W, stream_ptr())

    def reset(self) -> None:
        self.acc_real.zero_()
        self.acc_int.zero_()
        self.n_samples.zero_()

    def _read(self, sync_dist: bool):
        """one device read: ``(real, ints, n_samples)`` - the integers go behind the doubles as doubles (exact below
        2^53), so that ONE all-reduce sums both"""
        flat = torch.cat([self.acc_real.reshape(-1), self.acc_int.reshape(-1).double()])
        a, n = read(flat, self.n_samples.double(), sync_dist)
        nr = self.acc_real.numel()
        real = a[:nr].reshape(tuple(self.acc_real.shape)).copy()
        ints = np.rint(a[nr:]).astype(np.int64).reshape(tuple(self.acc_int.shape))
        return real, ints, np.rint(n).astype(np.int64)

    def counts(self, sync_dist: bool = False) -> dict:
        real, ints, n = self._read(sync_dist)
        return {"sums": real, "valid": ints[..., 0].copy(), "rank_counts": ints[..., 1:].copy(), "n_samples": n}

    def result(self, sync_dist: bool = False) -> dict:
        real, ints, n = self._read(sync_dist)
        return report(real, ints, n, self.band_w, self.members, self.names, self.bands)

    @staticmethod
    def table(result: dict, channel: str, band: Optional[str] = "global") -> str:
        """plain text: a row per lead with ``count`` and the seven ``METRICS``, then a row per lead of the rank
        histogram (``band=None``: the first band)"""
        names: List[str] = list(result["names"])
        bands: List[str] = list(result["bands"])
        if str(channel) not in names:
            raise ValueError(f"EnsembleCard.table: channel '{channel}' is not among the card's names")
        band = bands[0] if band is None else str(band)
        if band not in bands:
            raise ValueError(f"EnsembleCard.table: band '{band}' is not among the card's bands")
        c, r, M = names.index(str(channel)), bands.index(band), int(result["members"])
        lines = [f"{channel} / {band} / {M} members"]
        lines.append(f"{'lead':<6}{'count':>8}" + "".join(f"{m:>14}" for m in METRICS))
        n_leads = len(result["count"])
        for lead in range(n_leads):
            vals = "".join(f"{result[m][lead, c, r]:>14.5g}" for m in METRICS)
            lines.append(f"{lead:<6d}{int(result['count'][lead]):>8d}" + vals)
        lines.append("")
        lines.append(f"{'rank':<6}{'count':>8}" + "".join(f"{k:>8d}" for k in range(M + 1)))
        for lead in range(n_leads):
            vals = "".join(f"{result['rank_hist'][lead, c, r, k]:>8.4f}" for k in range(M + 1))
            lines.append(f"{lead:<6d}{int(result['count'][lead]):>8d}" + vals)
        return "\n".join(lines)
