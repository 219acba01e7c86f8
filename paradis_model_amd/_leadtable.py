"""What the per-lead verification tables share - ``verify.Scorecard``, ``spectrum.Spectra``, ``events.EventTable``,
``neighbourhood.FractionsTable``, ``ensemble.EnsembleCard``, ``probability.ProbabilityTable`` and ``seeps.SeepsTable``:
the argument checks of their constructors and of ``update``, the one-slot climatology index and the single device read
of ``result``.

Plain functions first; ``who`` is the class name that opens every message, so each table keeps its own words.  The small
base class ``LeadTable`` holds what the checks need (``names``, ``C``, ``n_leads``, ``device``, ``H``, ``W``, ``bands``,
``band_w``, ``climatology``, ``_ws``, ``_slot0``) and the phrases ``Forecaster.run`` refuses with.  Host only: nothing
here launches anything.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._tables import dense_state, sum_over_ranks


def names_and_leads(who: str, names: Sequence[str], n_leads) -> Tuple[List[str], int]:
    names = [str(n) for n in names]
    if len(names) < 1:
        raise ValueError(f"{who}: names must list at least one channel")
    return names, positive_int(who, "n_leads", n_leads)


def positive_int(who: str, what: str, n) -> int:
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f"{who}: {what} must be an integer >= 1, got {n!r}")
    return int(n)


def latitudes(who: str, lat_deg) -> np.ndarray:
    """``lat_deg`` as a float64 vector ``[H]``"""
    lat = torch.as_tensor(lat_deg).detach().reshape(-1).double().cpu().numpy()
    if lat.size < 1 or not np.isfinite(lat).all() or np.abs(lat).max() > 90.0:
        raise ValueError(f"{who}: lat_deg must be a vector [H] of finite latitudes in [-90, 90] degrees")
    return lat


def row_weights(who: str, lat: np.ndarray, weights=None) -> np.ndarray:
    """float64 ``[H]``: ``weights`` checked, or ``cos(lat)`` with the pole rows at 0"""
    if weights is None:
        w64 = np.clip(np.cos(np.deg2rad(lat)), 0.0, None)               # (cos(+-90 deg) in double is 6e-17, not 0)
        w64[np.abs(lat) == 90.0] = 0.0
        return w64
    w = torch.as_tensor(weights).detach().reshape(-1)
    if w.numel() != lat.size or not w.is_floating_point():
        raise ValueError(f"{who}: weights must be a floating-point vector [{lat.size}]")
    w64 = w.double().cpu().numpy()
    if not np.isfinite(w64).all() or (w64 < 0).any() or not w64.sum() > 0.0:
        raise ValueError(f"{who}: weights must be finite, >= 0 and not all zero")
    return w64


def band_weights(lat_deg, weights, bands, who: str = "Spectra") -> np.ndarray:
    """double ``[R, H]``: ``weights[h]`` where ``lat_lo <= lat_deg[h] <= lat_hi`` (inclusive), 0 elsewhere"""
    lat = np.asarray(lat_deg, np.float64).reshape(-1)
    w = np.asarray(weights, np.float64).reshape(-1)
    rows = []
    for name, edges in bands.items():
        try:
            lo, hi = (float(v) for v in edges)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: band '{name}' must be (lat_lo, lat_hi) in degrees, got {edges!r}") from None
        if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
            raise ValueError(f"{who}: band '{name}' must have finite lat_lo <= lat_hi, got {edges!r}")
        row = np.where((lat >= lo) & (lat <= hi), w, 0.0)
        if not row.sum() > 0.0:
            raise ValueError(f"{who}: band '{name}' {edges!r} holds no row of non-zero weight")
        rows.append(row)
    return np.ascontiguousarray(np.stack(rows))


def bands_to_weights(who: str, lat: np.ndarray, w64: np.ndarray, bands: Optional[dict]) -> Tuple[List[str], np.ndarray]:
    """(the band names, ``band_w`` double ``[R, H]`` on the host); default one band ``"global"``"""
    if bands is None:
        bands = {"global": (-90.0, 90.0)}
    if not isinstance(bands, dict) or len(bands) < 1:
        raise ValueError(f"{who}: bands must be a non-empty dict name -> (lat_lo, lat_hi)")
    return [str(b) for b in bands], band_weights(lat, w64, bands, who)


def climatology_tensor(who: str, it: str, cl, C: int, H: int, W: Optional[int], home: torch.device,
                       same_index: bool = False) -> torch.Tensor:
    """``cl`` is a contiguous float32 ``[K, C, H, W]`` (``W``: any when None) on ``home`` (``same_index``: on that very
    device, not only one of its type)"""
    if not isinstance(cl, torch.Tensor) or cl.dim() != 4 or cl.dtype != torch.float32 or cl.shape[0] < 1 or \
            cl.shape[1] != C or cl.shape[2] != H or (W is not None and cl.shape[3] != W) or not cl.is_contiguous():
        raise ValueError(f"{who}: climatology must be a contiguous float32 [K, {C}, {H}, {'W' if W is None else W}] "
                         f"tensor")
    if (cl.device != home) if same_index else (cl.device.type != home.type):
        raise ValueError(f"{who}: climatology lives on {cl.device}, {it} on {home}")
    return cl


def check_lead_and_forecast(who: str, it_has: str, n_leads: int, C: int, H: int, lead, forecast, truth,
                            n_lon: Optional[int] = None) -> Tuple[int, int]:
    """the lead, both tensors' rank and dtype and the forecast's shape ``[B, C, H, W]`` against a table of ``C``
    channels, ``H`` latitudes and - where the table was made for them - ``n_lon`` longitudes; returns ``(B, W)``.  What
    the truth's shape must be is the caller's: ``check_states`` or ``check_member_states``"""
    if isinstance(lead, bool) or not isinstance(lead, (int, np.integer)) or not 0 <= int(lead) < n_leads:
        raise ValueError(f"{who}.update: lead must be an integer in [0, {n_leads}), got {lead!r}")
    for what, t in (("forecast", forecast), ("truth", truth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{who}.update: {what} must be a [B, C, H, W] tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}.update: {what} must be float32, got {t.dtype}")
    B, Cf, Hf, W = forecast.shape
    if n_lon is None:
        if (Cf, Hf) != (C, H) or W < 1:
            raise ValueError(f"{who}.update: forecast is {tuple(forecast.shape)}; {it_has} {C} channels "
                             f"and {H} latitudes")
    elif (Cf, Hf, W) != (C, H, n_lon):
        raise ValueError(f"{who}.update: forecast is {tuple(forecast.shape)}; {it_has} {C} channels, "
                         f"{H} latitudes and {n_lon} longitudes")
    return B, W


def check_states(who: str, it_has: str, n_leads: int, C: int, H: int, lead, forecast, truth,
                 n_lon: Optional[int] = None) -> Tuple[int, int]:
    """the lead and the two ``[B, C, H, W]`` fp32 tensors of ``update`` against a table of ``C`` channels, ``H``
    latitudes and - where the table was made for them - ``n_lon`` longitudes; returns ``(B, W)``"""
    B, W = check_lead_and_forecast(who, it_has, n_leads, C, H, lead, forecast, truth, n_lon)
    if truth.shape != forecast.shape:
        raise ValueError(f"{who}.update: truth is {tuple(truth.shape)}, forecast {tuple(forecast.shape)}")
    return B, W


def check_member_states(who: str, it_has: str, n_leads: int, C: int, H: int, members: int, lead, forecast,
                        truth) -> Tuple[int, int]:
    """``check_states`` for a table of ensembles: forecast ``[G * members, C, H, W]``, member-minor, and ONE truth per
    ensemble, ``[G, C, H, W]``; returns ``(G, W)``"""
    B, W = check_lead_and_forecast(who, it_has, n_leads, C, H, lead, forecast, truth)
    if B % members != 0:
        raise ValueError(f"{who}.update: forecast is {tuple(forecast.shape)}: {B} states are not whole ensembles of "
                         f"{members} members")
    if tuple(truth.shape) != (B // members, C, H, W):
        raise ValueError(f"{who}.update: truth is {tuple(truth.shape)}, forecast {tuple(forecast.shape)}: "
                         f"{B // members} ensembles of {members} members need truth {(B // members, C, H, W)}")
    return B // members, W


def check_clim_index(who: str, it_has: str, climatology, clim_index, B: int, W: int) -> None:
    """the ``clim_index`` rules of ``update``: none without a climatology, optional with one slot, else int32 ``[B]``"""
    if climatology is None:
        if clim_index is not None:
            raise ValueError(f"{who}.update: clim_index given, but {it_has} no climatology")
        return
    if climatology.shape[3] != W:
        raise ValueError(f"{who}.update: forecast has {W} longitudes, the climatology {climatology.shape[3]}")
    if clim_index is None:
        if climatology.shape[0] != 1:
            raise ValueError(f"{who}.update: clim_index is needed to choose among the {climatology.shape[0]} "
                             f"climatology slots")
    elif not isinstance(clim_index, torch.Tensor) or clim_index.dtype != torch.int32 or tuple(clim_index.shape) != (B,):
        raise ValueError(f"{who}.update: clim_index must be an int32 tensor [{B}]")


def resolve_clim_index(who: str, slot0: Dict[int, torch.Tensor], climatology, clim_index, B: int, device):
    """the dense ``[B]`` int32 index on the device that goes to the entry point (None without a climatology); the index
    of a one-slot climatology is a cached row of zeros"""
    if climatology is None:
        return None
    if clim_index is None:
        if B not in slot0:
            with torch.inference_mode(False):
                slot0[B] = torch.zeros(B, dtype=torch.int32, device=device)
        clim_index = slot0[B]
    if not clim_index.is_cuda:
        raise ValueError(f"{who}.update: clim_index must live on the device")
    return clim_index.contiguous()                   # a column of [B, n_stored] becomes dense; no host wait


def read(acc: torch.Tensor, counts: torch.Tensor, sync_dist: bool) -> Tuple[np.ndarray, np.ndarray]:
    """``(acc, counts)`` on the host as numpy: one tensor - the accumulators and, behind them, the counts -, so one
    all-reduce (``sync_dist``) and one device read"""
    flat = sum_over_ranks(torch.cat([acc.reshape(-1), counts]), sync_dist).numpy()
    return flat[:acc.numel()].reshape(tuple(acc.shape)), flat[acc.numel():].copy()


class LeadTable:
    """The base of the per-lead tables.  A subclass states how messages call it (``IT`` / ``IT_HAS``: "the table" /
    "the table has") and how ``Forecaster.run`` does (``NOUN``, ``HAS``, ``NEEDS``), and whether its ``update`` takes a
    ``clim_index`` and how many batch entries share one truth (``members``: 1, or an ensemble table's own); its
    constructor calls ``__init__``, then ``_set_grid`` and ``_set_climatology`` as far as it has latitudes, bands and a
    climatology, in the order its checks fire."""
    IT = IT_HAS = NOUN = HAS = NEEDS = ""
    TAKES_CLIM_INDEX = True
    members = 1

    def __init__(self, names: Sequence[str], n_leads: int, device):
        self.who = type(self).__name__
        self.names, self.n_leads = names_and_leads(self.who, names, n_leads)
        self.all_names = self.names                   # the channels of a state (``_set_channels`` narrows ``names``)
        self.C = len(self.names)
        self.device = torch.device(device)
        self.H: Optional[int] = None
        self.W: Optional[int] = None                  # longitudes, once known
        self.climatology: Optional[torch.Tensor] = None
        self._ws: Dict[tuple, torch.Tensor] = {}      # (device, stream) -> workspace
        self._slot0: Dict[int, torch.Tensor] = {}     # B -> zeros [B] int32: the index of a one-slot climatology

    def _set_grid(self, lat_deg, weights, bands) -> np.ndarray:
        """``H``, ``bands`` and ``band_w`` (double ``[R, H]``, on the host); returns the latitudes"""
        lat = latitudes(self.who, lat_deg)
        self.H = lat.size
        self.bands, self.band_w = bands_to_weights(self.who, lat, row_weights(self.who, lat, weights), bands)
        return lat

    def _set_channels(self, channels) -> None:
        """``names`` narrowed to the subset ``channels`` (by name, in the order given; None: all) and ``index``, their
        positions in a state; ``all_names`` stays the state's names"""
        chosen = self.all_names if channels is None else [str(c) for c in channels]
        if len(chosen) < 1:
            raise ValueError(f"{self.who}: channels must name at least one channel")
        for c in chosen:
            if c not in self.all_names:
                raise ValueError(f"{self.who}: channel '{c}' is not among the names")
        if len(set(chosen)) != len(chosen):
            raise ValueError(f"{self.who}: channels must not repeat a name")
        self.names = chosen
        self.index = [self.all_names.index(c) for c in chosen]

    def _set_climatology(self, climatology, home=None, same_index: bool = False) -> None:
        if climatology is not None:
            self.climatology = climatology_tensor(self.who, self.IT, climatology, self.C, self.H, self.W,
                                                  self.device if home is None else home, same_index)

    def _check_longitudes(self, W: int) -> None:
        """what a table refuses about the longitudes of an ``update`` beyond the shared checks"""

    def _check(self, lead, forecast, truth, clim_index=None, n_lon: Optional[int] = None):
        """argument checks of ``update``; returns (B, C, H, W)"""
        B, W = check_states(self.who, self.IT_HAS, self.n_leads, self.C, self.H, lead, forecast, truth, n_lon)
        self._check_longitudes(W)
        dense_state(forecast, "forecast", f"{self.who}.update")
        dense_state(truth, "truth", f"{self.who}.update")
        if self.TAKES_CLIM_INDEX:
            check_clim_index(self.who, self.IT_HAS, self.climatology, clim_index, B, W)
        return B, self.C, self.H, W

    def _clim_args(self, clim_index, forecast):
        """``(clim_index on the device or None, K)`` for the entry point"""
        idx = resolve_clim_index(self.who, self._slot0, self.climatology, clim_index, forecast.shape[0], forecast.device)
        return idx, 0 if idx is None else self.climatology.shape[0]
