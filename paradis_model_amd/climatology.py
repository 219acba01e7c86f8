"""The verification climatology, built on the device from a ``dataset.DeviceStore``: the ``clim [K, C, H, W]`` tensor and
the slot index per sample that ``verify.Scorecard`` needs for the anomaly correlation (ACC) and the activity.

Definition (``ClimPlan``).  A slot is a (day of year, hour of day) pair.  A store row at time ``t`` whose hour of day
``h`` is one of the plan's hours contributes, for every integer ``d`` in ``[-half, half]`` (``half = window_days // 2``),
to the slot (dayofyear(``t + d`` days), ``h``) with weight ``w(d)``: 1 (``"boxcar"``) or ``exp(-d^2 / (2 sigma_days^2))``
(``"gaussian"``).  The day-of-year arithmetic is calendar-exact (numpy ``datetime64``): the window wraps over New Year
and over 29 February without a fixed circle length, and day 366 receives rows only from around leap years' 31 December.  The
slot's value is the weighted mean over its entries, per pixel, with NaN and +-Inf skipped (a packed store's "missing"
decodes to NaN): the rule of ``prepare.StoreStats``.  This is the project's OWN definition.  It follows the spirit of
WeatherBench-2's windowed day-of-year x hour climatology, but it is not pinned against it, and no WeatherBench-2 file
is read.

``build`` runs one launch of ``csrc/climatology.hip`` over the store as it is held - float32 or 16-bit packed, decoded
inside the launch - and, with a ``forecast.PostSpec`` whose ``winds`` is set, one small launch that turns the means of
the Cartesian wind triples into ``u, v, w`` by the expression of the forecast post-processing (``csrc/winds.h``).  The
rotation that gives ``u`` and ``v`` is linear per pixel, so rotating the mean equals the mean of the rotated winds up to
rounding; ``w`` of a pressure level also divides by the level's temperature, so it is the ``w`` of the MEAN state (mean
Cartesian wind, mean temperature), which differs from the mean of the rows' ``w`` in second order of the temperature's
relative variation.

``build_quantiles`` gives, for the same lists, per-cell QUANTILES instead of the mean (``csrc/quantile.hip``; the
definition is in its docstring): the per-cell thresholds of ``events.EventTable``, ``neighbourhood.FractionsTable`` and
``probability.ProbabilityTable``, which take ``QuantileClimatology.field(...)`` as their ``climatology=`` and
``quantile_event(name)`` as an event.

``build_seeps`` gives, for the same lists again, the SEEPS climatology (the same kernel's second selection stage; the
definition is in its docstring): per cell the fraction of dry values and a quantile of the wet ones, what
``seeps.SeepsTable`` takes as its ``climatology=``.

No CPU fallback: ``build``, ``build_quantiles`` and ``build_seeps`` need the store on the HIP device.  ``ClimPlan`` is
host-only.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr

US_PER_HOUR = 3600 * 1000000
US_PER_DAY = 24 * US_PER_HOUR


def _as_us(times_us) -> np.ndarray:
    if isinstance(times_us, torch.Tensor):
        times_us = times_us.detach().cpu().numpy()
    a = np.asarray(times_us)
    if a.dtype.kind == "M":
        a = a.astype("datetime64[us]").astype(np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"times must be int64 microseconds (feed.times_to_us) or datetime64, got {a.dtype}")
    return a.astype(np.int64)


def _day_hour(us: np.ndarray):
    """(day of year 1..366, hour of day, whole-hour mask) of int64 microseconds, any shape; calendar-exact"""
    days = np.floor_divide(us, US_PER_DAY)
    rest = us - days * US_PER_DAY
    return _day_of_year(days), rest // US_PER_HOUR, rest % US_PER_HOUR == 0


def _day_of_year(days: np.ndarray) -> np.ndarray:
    """day of year (1..366) of int64 days since 1970-01-01"""
    d = days.astype("datetime64[D]")
    return (d - d.astype("datetime64[Y]").astype("datetime64[D]")).astype(np.int64) + 1


def _first_time(us: np.ndarray, bad: np.ndarray) -> str:
    return str(us.reshape(-1)[np.flatnonzero(bad.reshape(-1))[0]].astype("datetime64[us]"))


class ClimPlan:
    """The host plan of a climatology: which store rows contribute to which slot, with which weight (module docstring
    for the definition).  Needs no GPU.

    ``times_us``: the store's ``[T]`` int64 microseconds (``DeviceStore.times_us``, ``feed.times_to_us``).  ``start`` /
    ``end``: dates as ``DeviceDataset`` takes them (a date without a clock is ``T00:00:00`` / ``T23:59:59``); only rows
    inside contribute - this is how test years stay out of the climatology.  ``hours``: the hours of day that form
    slots, kept sorted; default: the distinct hours of day among the contributing rows.  A contributing row off the
    whole hour is refused; one whose hour is not in ``hours`` is left out.  ``days``: the days of year (1..366) to
    build, default all 366 (a 0.25 degree climatology of all 366 x 4 slots does not fit in memory).  ``window_days``:
    odd, 1..365.  ``weights``: ``"boxcar"`` or ``"gaussian"`` (with ``sigma_days > 0``).

    ``K = len(days) * len(hours)``; the slot of (day ``d``, hour ``h``) is ``days.index(d) * len(hours) +
    hours.index(h)``.  ``lists()``: the CSR tables ``(ptr int64 [K + 1], rows int64 [N], w float64 [N])``; the entries
    of a slot are sorted by row ascending, which is the summation order.  ``entries`` ``[K]``: entries per slot (a slot
    may be empty: its climatology is NaN).  ``slot_of(times_us)``: the int32 slots of valid times, any shape."""

    def __init__(self, times_us, *, start=None, end=None, hours: Optional[Sequence[int]] = None,
                 days: Optional[Sequence[int]] = None, window_days: int = 1, weights: str = "boxcar",
                 sigma_days: Optional[float] = None):
        from .dataset import _date_us
        t = _as_us(times_us).reshape(-1)
        self.times_us = t
        if isinstance(window_days, bool) or int(window_days) != window_days or int(window_days) < 1 or \
                int(window_days) % 2 == 0 or int(window_days) > 365:
            raise ValueError(f"ClimPlan: window_days must be an odd integer in [1, 365], got {window_days!r}")
        self.window_days = int(window_days)
        if weights not in ("boxcar", "gaussian"):
            raise ValueError(f"ClimPlan: weights must be 'boxcar' or 'gaussian', got {weights!r}")
        if weights == "gaussian":
            if sigma_days is None or not np.isfinite(float(sigma_days)) or float(sigma_days) <= 0.0:
                raise ValueError(f"ClimPlan: weights='gaussian' needs sigma_days > 0, got {sigma_days!r}")
        elif sigma_days is not None:
            raise ValueError("ClimPlan: sigma_days goes with weights='gaussian'")
        self.weights, self.sigma_days = weights, None if sigma_days is None else float(sigma_days)
        self.start_us = None if start is None else _date_us(start, "T00:00:00")
        self.end_us = None if end is None else _date_us(end, "T23:59:59")
        keep = np.ones(t.shape, bool)
        if self.start_us is not None:
            keep &= t >= self.start_us
        if self.end_us is not None:
            keep &= t <= self.end_us
        _, hour, whole = _day_hour(t)
        if bool((keep & ~whole).any()):
            raise ValueError(f"ClimPlan: the store row at {_first_time(t, keep & ~whole)} is not on a whole hour")
        if hours is None:
            hours = np.unique(hour[keep]).tolist()
        self.hours = sorted(int(h) for h in hours)
        if len(set(self.hours)) != len(self.hours) or any(not 0 <= h <= 23 for h in self.hours) or \
                any(int(h) != h for h in hours):
            raise ValueError(f"ClimPlan: hours must be distinct integers in [0, 23], got {list(hours)}")
        self.days = [int(d) for d in (range(1, 367) if days is None else days)]
        if len(set(self.days)) != len(self.days) or any(not 1 <= d <= 366 for d in self.days):
            raise ValueError("ClimPlan: days must be distinct days of year in [1, 366]")
        self._day_pos = np.full(367, -1, np.int64)
        self._day_pos[self.days] = np.arange(len(self.days))
        self._hour_pos = np.full(24, -1, np.int64)
        self._hour_pos[self.hours] = np.arange(len(self.hours))
        self.n_slots = K = len(self.days) * len(self.hours)

        # every (row, delta) pair in row-major order; a stable sort by slot then leaves each slot's rows ascending
        # (window_days <= 365: the dates t + delta of one row are less than a year apart, so a row meets a slot once)
        half = self.window_days // 2
        delta = np.arange(-half, half + 1, dtype=np.int64)
        # (math.exp per offset, not numpy's vectorised exp, whose last bit depends on the build's SIMD kernels)
        wd = np.array([1.0 if weights == "boxcar" else math.exp(-(d * d) / (2.0 * self.sigma_days * self.sigma_days))
                       for d in delta.tolist()], np.float64)
        rows = np.flatnonzero(keep & (self._hour_pos[np.clip(hour, 0, 23)] >= 0))
        day0 = np.floor_divide(t[rows], US_PER_DAY)
        doy = _day_of_year(day0[:, None] + delta[None, :])                       # [n, D]
        slot = self._day_pos[doy] * len(self.hours) + self._hour_pos[hour[rows]][:, None]
        ok = self._day_pos[doy] >= 0
        slot, row, w = slot[ok], np.broadcast_to(rows[:, None], doy.shape)[ok], np.broadcast_to(wd, doy.shape)[ok]
        order = np.argsort(slot, kind="stable")
        self._rows = np.ascontiguousarray(row[order], np.int64)
        self._w = np.ascontiguousarray(w[order], np.float64)
        self.entries = np.bincount(slot, minlength=K).astype(np.int64) if K else np.zeros(0, np.int64)
        self._ptr = np.concatenate([[0], np.cumsum(self.entries)]).astype(np.int64)

    def lists(self):
        """``(ptr [K + 1] int64, rows [N] int64, w [N] float64)``: the CSR tables of ``paradis_clim_mean``"""
        return self._ptr, self._rows, self._w

    def slot_of(self, times_us) -> np.ndarray:
        """the slot of each valid time (int32, the same shape); ``ValueError`` naming the first time whose day or hour
        was not built, or which is off the whole hour"""
        t = _as_us(times_us)
        doy, hour, whole = _day_hour(t)
        day_pos, hour_pos = self._day_pos[doy], self._hour_pos[np.clip(hour, 0, 23)]
        bad = ~whole | (day_pos < 0) | (hour_pos < 0)
        if bool(bad.any()):
            raise ValueError(f"ClimPlan.slot_of: no slot was built for {_first_time(t, bad)} (days of year "
                             f"{len(self.days)} of 366, hours {self.hours})")
        return (day_pos * len(self.hours) + hour_pos).astype(np.int32)


def clim_mean(store, ptr: torch.Tensor, rows: torch.Tensor, w: torch.Tensor, cols: torch.Tensor,
              out: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None):
    """The launch over whatever the store holds: ``paradis_clim_mean`` for a float32 store, ``paradis_clim_mean_packed``
    for a packed one.  Device tables ``ptr`` int64 ``[K + 1]``, ``rows`` int64 ``[N]``, ``w`` float64 ``[N]``, ``cols``
    int32 ``[C]``; returns ``(out [K, C, H, W] float32, flag [1] int32)``.  No host synchronisation; a row, column or
    list bound outside the store or the lists is clamped and raises ``flag``.  ``build`` is the public way in."""
    T, F, H, W = store.shape
    dev = store.device
    require_hip(store.data if store.packing is None else store.plane_params, out)
    K, C, N = int(ptr.numel()) - 1, int(cols.numel()), int(rows.numel())
    for name, t, dtype in (("ptr", ptr, torch.int64), ("rows", rows, torch.int64), ("w", w, torch.float64),
                           ("cols", cols, torch.int32)):
        if t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"clim_mean: {name} must be a contiguous 1-D {dtype} tensor on {dev}")
    if K < 0 or int(w.numel()) != N:
        raise ValueError("clim_mean: ptr needs K + 1 entries, rows and w one per list entry")
    if out is None:
        out = torch.empty(K, C, H, W, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (K, C, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"clim_mean: out must be contiguous float32 {(K, C, H, W)} on {dev}")
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tail = (T, F, H, W, dptr(ptr), dptr(rows), dptr(w), N, K, dptr(cols), C, dptr(out), dptr(flag), stream_ptr())
    P = H * W
    if store.packing is None:
        _lib.call("clim_mean", 4.0 * N * C * P + 4.0 * K * C * P, dptr(store.data), *tail)
    else:
        _lib.call("clim_mean_packed", 2.0 * N * C * P + 4.0 * K * C * P, dptr(store.codes), dptr(store.plane_params),
                  dptr(store.domain_dev), *tail)
    return out, flag


def spherical_winds_inplace(data: torch.Tensor, spec, lat_deg, lon_deg) -> torch.Tensor:
    """``paradis_spherical_winds_inplace``: the ``(x, y, z)`` planes of every wind triple ``spec`` (a
    ``forecast.PostSpec``) found - ``spec.ix / iy / iz`` per level, ``spec.sfc`` - of ``data [K, C, H, W]`` (physical
    units, contiguous float32 on the device) become ``(u, v, w)``, in place; one launch, no host synchronisation.  The
    expression is ``forecast.postprocess``'s (one ``__device__`` function, the same bits): fp64 from the fp32 values and
    the double sin / cos tables of ``_tables.trig_tables``, rounded once.  A level's ``w`` reads that level's temperature
    channel.  A NaN in any component of a triple gives NaN in all three.  Returns ``data``."""
    require_hip(data)
    if data.dim() != 4 or not data.is_contiguous():
        raise ValueError("spherical_winds_inplace: data must be a contiguous [K, C, H, W] tensor")
    K, C, H, W = (int(v) for v in data.shape)
    if C != spec.num_channels:
        raise ValueError(f"spherical_winds_inplace: data has {C} channels, the spec {spec.num_channels}")
    if not spec.winds:
        raise ValueError("spherical_winds_inplace: the spec was built with winds=False")
    trig, th, tw = spec.trig_tables(lat_deg, lon_deg, data.device)
    if (th, tw) != (H, W):
        raise ValueError(f"spherical_winds_inplace: lat/lon of {th} x {tw} points for {H} x {W} fields")
    _, _, _, units, plev = spec.device_tables(data.device)
    host = np.ascontiguousarray(spec.units, np.int32)
    n_triples = len(spec.ix) + (1 if spec.sfc else 0)
    _lib.call("spherical_winds_inplace", 28.0 * K * n_triples * H * W, dptr(data), dptr(units), host.ctypes.data,
              host.shape[0], dptr(plev), spec.num_levels, dptr(trig), K, C, H, W, stream_ptr())
    return data


class Climatology:
    """What ``build`` returns.  ``data``: ``[K, C, H, W]`` float32 on the store's device, channel order ``names``
    (``PostSpec.names``; ``u, v, w`` where the wind triples were, when built with winds) - what
    ``verify.Scorecard(..., climatology=clim.data)`` takes as it is.  ``index(times_us)``: the slots of valid times as an
    int32 tensor of the same shape on the device - ``Scorecard.update``'s ``clim_index`` for ``[B]`` times,
    ``Forecaster.run``'s for ``[B, n_stored]``.  ``plan``, ``names``, ``winds``."""

    def __init__(self, data: torch.Tensor, plan: ClimPlan, names, winds: bool):
        self.data, self.plan, self.names, self.winds = data, plan, list(names), bool(winds)

    def index(self, times_us) -> torch.Tensor:
        return torch.from_numpy(self.plan.slot_of(times_us)).to(self.data.device)


def build(store, plan: ClimPlan, spec=None, *, names: Optional[Sequence[str]] = None,
          winds: Optional[bool] = None) -> Climatology:
    """The climatology of ``store`` (a ``dataset.DeviceStore`` on the HIP device, float32 or packed; never written) by
    ``plan``, in the channel layout of ``spec`` (a ``forecast.PostSpec``): channel ``c`` is the store feature named
    ``spec.names[c]``, in physical units, and with ``spec.winds`` every wind triple is turned into ``u, v, w``.  Without
    a spec: ``names=[...]`` and ``winds=False``.  ``winds=False`` beside a spec keeps the Cartesian means.

    One launch of ``paradis_clim_mean`` (``N*C*H*W*(4 | 2)`` bytes read, ``K*C*H*W*4`` written; bit-identical run to
    run), one of ``paradis_spherical_winds_inplace``, and one read of the launch's flag word.  Refused: a CPU store, a
    plan made for other times, a name the store does not hold (named in the error), winds without a spec."""
    if spec is None and names is None:
        raise ValueError("climatology.build: a PostSpec or names=[...] is needed")
    if spec is not None and names is not None and list(names) != list(spec.names):
        raise ValueError("climatology.build: names differ from spec.names")
    names = [str(n) for n in (spec.names if spec is not None else names)]
    winds = (spec is not None and spec.winds) if winds is None else bool(winds)
    if winds and (spec is None or not spec.winds):
        raise ValueError("climatology.build: winds=True needs a PostSpec built with winds=True")
    if not np.array_equal(plan.times_us, store.times_us.numpy()):
        raise ValueError("climatology.build: the plan was made for other times than the store's times_us")
    column = {name: j for j, name in enumerate(store.features)}
    for name in names:
        if name not in column:
            raise ValueError(f"climatology.build: channel '{name}' is not among the store's features")
    if torch.device(store.device).type == "cpu":
        raise ValueError("climatology.build: the climatology is built on the HIP device (no CPU fallback); got a CPU "
                         "store")
    dev = store.device
    ptr, rows, w = (torch.from_numpy(a).to(dev) for a in plan.lists())
    cols = torch.tensor([column[n] for n in names], dtype=torch.int32, device=dev)
    data, flag = clim_mean(store, ptr, rows, w, cols)
    if winds:
        spherical_winds_inplace(data, spec, store.lat, store.lon)
    if int(flag.item()):
        raise RuntimeError("climatology.build: a list entry fell outside the store (clamped by the kernel)")
    return Climatology(data, plan, names, winds)


# ---------------------------------------------------------------------------------- quantiles
def max_quantile_entries() -> int:
    """the longest slot list ``clim_quantile`` takes (``paradis_clim_quantile_max_entries()``)"""
    return int(_lib.lib.paradis_clim_quantile_max_entries())


def _levels(who: str, q) -> np.ndarray:
    """1 to 8 distinct levels in [0, 1] as float64"""
    try:
        a = np.asarray([q] if np.isscalar(q) else list(q), np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: q must be a number or a list of numbers in [0, 1], got {q!r}") from None
    if not 1 <= a.size <= 8:
        raise ValueError(f"{who}: {a.size} levels, 1 to 8 go into one launch")
    bad = ~((a >= 0.0) & (a <= 1.0))
    if bool(bad.any()):
        raise ValueError(f"{who}: level {a[np.flatnonzero(bad)[0]]!r} is outside [0, 1]")
    if np.unique(a).size != a.size:
        dup = [float(v) for v in a if int((a == v).sum()) > 1][0]
        raise ValueError(f"{who}: level {dup!r} is given twice")
    return np.ascontiguousarray(a)


def clim_quantile(store, ptr: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor, q, *,
                  max_entries: Optional[int] = None, min_count: int = 1, out: Optional[torch.Tensor] = None,
                  flag: Optional[torch.Tensor] = None):
    """The launch over whatever the store holds: ``paradis_clim_quantile`` for a float32 store,
    ``paradis_clim_quantile_packed`` for a packed one.  Device tables ``ptr`` int64 ``[K + 1]``, ``rows`` int64 ``[N]``,
    ``cols`` int32 ``[C]`` as ``clim_mean`` takes them; ``q``: 1 to 8 distinct levels in [0, 1] (host).  Returns ``(out
    [Q, K, C, H, W] float32, flag [1] int32)``.  No host synchronisation: ``max_entries``, the longest list, is the
    caller's knowledge (``ClimPlan.entries.max()``); it fixes the tile, and without it the launch takes the tile of the
    longest list supported (``max_quantile_entries()``, the slowest).  A list longer than ``max_entries`` is cut to its
    first ``max_entries`` entries and raises ``flag``, as a row, column or list bound outside the store does.
    ``build_quantiles`` is the public way in."""
    T, F, H, W = store.shape
    dev = store.device
    require_hip(store.data if store.packing is None else store.plane_params, out)
    K, C, N = int(ptr.numel()) - 1, int(cols.numel()), int(rows.numel())
    for name, t, dtype in (("ptr", ptr, torch.int64), ("rows", rows, torch.int64), ("cols", cols, torch.int32)):
        if t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"clim_quantile: {name} must be a contiguous 1-D {dtype} tensor on {dev}")
    if K < 0:
        raise ValueError("clim_quantile: ptr needs K + 1 entries")
    levels = _levels("clim_quantile", q)
    Q = int(levels.size)
    longest = max_quantile_entries()
    max_entries = longest if max_entries is None else int(max_entries)
    if not 0 <= max_entries <= longest:
        raise ValueError(f"clim_quantile: max_entries must lie in [0, {longest}], got {max_entries}")
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError(f"clim_quantile: min_count must be an integer >= 1, got {min_count!r}")
    if out is None:
        out = torch.empty(Q, K, C, H, W, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (Q, K, C, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"clim_quantile: out must be contiguous float32 {(Q, K, C, H, W)} on {dev}")
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tail = (T, F, H, W, dptr(ptr), dptr(rows), N, K, max_entries, dptr(cols), C, levels.ctypes.data, Q, int(min_count),
            dptr(out), dptr(flag), stream_ptr())
    P = H * W
    if store.packing is None:
        _lib.call("clim_quantile", 4.0 * N * C * P + 4.0 * Q * K * C * P, dptr(store.data), *tail)
    else:
        _lib.call("clim_quantile_packed", 2.0 * N * C * P + 4.0 * Q * K * C * P, dptr(store.codes),
                  dptr(store.plane_params), dptr(store.domain_dev), *tail)
    return out, flag


class QuantileClimatology:
    """What ``build_quantiles`` returns.  ``data``: ``[Q, K, C, H, W]`` float32 on the store's device, compact over the
    chosen ``names`` (physical units; NaN where a cell kept fewer than ``min_count`` values); ``levels``: the ``Q``
    levels as floats; ``plan``.

    ``index(times_us)``: as ``Climatology.index``.  ``level(q)``: the ``[K, C, H, W]`` view of one level.
    ``field(state_names, levels)``: a new ``[K, len(state_names), H, W]`` tensor in a state's channel layout, in which
    channel ``name`` holds the level ``levels[name]`` (a dict name -> q) and every other plane is NaN, so that an anomaly
    source on such a channel counts no cell - what ``EventTable``, ``FractionsTable`` and ``ProbabilityTable`` take as
    ``climatology=`` beside ``quantile_event(name)``.  Plain indexing, no kernel.  A table holds ONE climatology, so two
    levels of the same channel (q10 and q90 of temperature) need two fields and two tables."""

    def __init__(self, data: torch.Tensor, plan: ClimPlan, names, levels, min_count: int = 1):
        self.data, self.plan, self.names = data, plan, list(names)
        self.levels = [float(v) for v in levels]
        self.min_count = int(min_count)

    def index(self, times_us) -> torch.Tensor:
        return torch.from_numpy(self.plan.slot_of(times_us)).to(self.data.device)

    def _level_pos(self, who: str, q) -> int:
        try:
            return self.levels.index(float(q))
        except (TypeError, ValueError):
            raise ValueError(f"QuantileClimatology.{who}: level {q!r} was not built (levels {self.levels})") from None

    def level(self, q) -> torch.Tensor:
        return self.data[self._level_pos("level", q)]

    def field(self, state_names: Sequence[str], levels: dict) -> torch.Tensor:
        state_names = [str(n) for n in state_names]
        if not isinstance(levels, dict) or not levels:
            raise ValueError("QuantileClimatology.field: levels must be a non-empty dict name -> q")
        _, K, _, H, W = self.data.shape
        out = torch.full((K, len(state_names), H, W), float("nan"), dtype=torch.float32, device=self.data.device)
        for name, q in levels.items():
            if name not in state_names:
                raise ValueError(f"QuantileClimatology.field: '{name}' is not among the state's names")
            if name not in self.names:
                raise ValueError(f"QuantileClimatology.field: no quantiles were built for '{name}'")
            out[:, state_names.index(name)] = self.data[self._level_pos("field", q), :, self.names.index(name)]
        return out


def quantile_event(name: str, direction: str = "ge") -> dict:
    """The events-dict entry of "``name`` beyond its per-cell quantile": ``{"source": ("anomaly", name), "thresholds":
    [0.0], "direction": direction}`` for a table whose ``climatology=`` is ``QuantileClimatology.field(...)``.  The
    anomaly ``x - q`` of two finite fp32 values is zero only when they are equal (no flush to zero), so ``x - q >= 0``
    decides exactly ``x >= q`` (``"le"``: ``x <= q``)."""
    if direction not in ("ge", "le"):
        raise ValueError(f"quantile_event: direction must be 'ge' or 'le', got {direction!r}")
    return {"source": ("anomaly", str(name)), "thresholds": [0.0], "direction": direction}


def build_quantiles(store, plan: ClimPlan, q, spec=None, *, names: Optional[Sequence[str]] = None,
                    min_count: int = 1) -> QuantileClimatology:
    """The quantile climatology of ``store`` (a ``dataset.DeviceStore`` on the HIP device, float32 or packed; never
    written) by ``plan``, at the levels ``q`` (1 to 8 distinct numbers in [0, 1]), for the channels ``names`` (default
    ``spec.names``), in physical units.

    Definition (the project's OWN, like ``ClimPlan``'s; not pinned against any package).  For slot ``k``, channel ``c``
    and cell ``p``: the values ``x[rows[j], col[c], p]`` over the slot's list entries ``j``, UNWEIGHTED; ``-0.0`` is read
    as ``+0.0``; NaN and +-Inf are skipped (the rule of ``clim_mean`` and ``StoreStats``).  With ``m`` values kept,
    ``v[0] <= ... <= v[m-1]`` ascending, and a level ``q``::

        pos = q * (m - 1);  lo = floor(pos);  hi = min(lo + 1, m - 1);  frac = pos - lo
        out = float32(v[lo] + (v[hi] - v[lo]) * frac)        in double, one rounding
        out = NaN   when m < min_count   (min_count >= 1)

    numpy's ``method="linear"`` position rule with the plain lerp (numpy changes its lerp form at ``frac >= 0.5``, which
    moves a rare result by one float32 ulp).

    One launch of ``paradis_clim_quantile`` (``csrc/quantile.hip``: keys in LDS, a bitonic sort per cell; bit-identical
    run to run) and one read of the launch's flag word.  Refused: what ``build`` refuses (a CPU store, a plan made for
    other times, a name the store does not hold); a plan with ``weights="gaussian"`` (quantiles are unweighted); bad
    levels; a slot whose list is longer than ``max_quantile_entries()``; and, with a ``PostSpec`` built with
    ``winds=True``, any name of a wind triple - the quantile of a Cartesian component is not the quantile of ``u`` or
    ``v``: pass ``names=`` without the winds."""
    who = "climatology.build_quantiles"
    if spec is None and names is None:
        raise ValueError(f"{who}: a PostSpec or names=[...] is needed")
    names = [str(n) for n in (spec.names if names is None else names)]
    if spec is not None:
        for name in names:
            if name not in spec.names:
                raise ValueError(f"{who}: channel '{name}' is not among spec.names")
        if spec.winds:
            wind = {spec.names[c] for c in list(spec.ix) + list(spec.iy) + list(spec.iz) + list(spec.sfc)}
            for name in names:
                if name in wind:
                    raise ValueError(f"{who}: '{name}' belongs to a wind triple of a spec built with winds=True; the "
                                     f"quantile of a Cartesian component is not the quantile of u or v: pass names= "
                                     f"without the winds")
    if plan.weights != "boxcar":
        raise ValueError(f"{who}: the plan has weights='{plan.weights}', but quantiles are unweighted: make the plan "
                         f"with weights='boxcar'")
    levels = _levels(who, q)
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError(f"{who}: min_count must be an integer >= 1, got {min_count!r}")
    if not np.array_equal(plan.times_us, store.times_us.numpy()):
        raise ValueError(f"{who}: the plan was made for other times than the store's times_us")
    column = {name: j for j, name in enumerate(store.features)}
    for name in names:
        if name not in column:
            raise ValueError(f"{who}: channel '{name}' is not among the store's features")
    longest = int(plan.entries.max()) if plan.entries.size else 0
    if longest > max_quantile_entries():
        k = int(np.argmax(plan.entries))
        raise ValueError(f"{who}: slot {k} (day of year {plan.days[k // len(plan.hours)]}, hour "
                         f"{plan.hours[k % len(plan.hours)]}) has {longest} entries, at most {max_quantile_entries()} "
                         f"can be sorted per cell: a shorter window or fewer years")
    if torch.device(store.device).type == "cpu":
        raise ValueError(f"{who}: the quantiles are built on the HIP device (no CPU fallback); got a CPU store")
    dev = store.device
    ptr, rows, _ = plan.lists()
    ptr, rows = torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev)
    cols = torch.tensor([column[n] for n in names], dtype=torch.int32, device=dev)
    data, flag = clim_quantile(store, ptr, rows, cols, levels, max_entries=longest, min_count=int(min_count))
    if int(flag.item()):
        raise RuntimeError(f"{who}: a list entry fell outside the store (clamped by the kernel)")
    return QuantileClimatology(data, plan, names, levels, int(min_count))


# ---------------------------------------------------------------------------------- SEEPS
def _dry_threshold(who: str, dry) -> float:
    """a finite number that stays finite in float32, as the float the kernel gets"""
    try:
        with np.errstate(over="ignore"):
            d = np.float32(dry)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: dry_threshold must be a finite number, got {dry!r}") from None
    if isinstance(dry, bool) or not np.isfinite(d):
        raise ValueError(f"{who}: dry_threshold must be a finite number (in float32), got {dry!r}")
    return float(d)


def _wet_level(who: str, wet_level) -> float:
    try:
        q = float(wet_level)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: wet_level must be a number in [0, 1], got {wet_level!r}") from None
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"{who}: wet_level {wet_level!r} is outside [0, 1]")
    return q


def clim_seeps(store, ptr: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor, dry, *, wet_level: float = 2.0 / 3.0,
               max_entries: Optional[int] = None, min_count: int = 1, out: Optional[torch.Tensor] = None,
               flag: Optional[torch.Tensor] = None):
    """The launch over whatever the store holds: ``paradis_clim_seeps`` for a float32 store, ``paradis_clim_seeps_packed``
    for a packed one - ``clim_quantile``'s twin: the same tables, ``max_entries``, ``min_count``, clamp and ``flag``,
    with ``dry`` (a finite number, rounded to float32) and ``wet_level`` (in [0, 1]) in place of the levels.  Returns
    ``(out [2, K, C, H, W] float32, flag [1] int32)``: plane 0 the dry fraction ``p1``, plane 1 the ``wet_level``
    quantile of the wet values.  No host synchronisation.  ``build_seeps`` is the public way in."""
    T, F, H, W = store.shape
    dev = store.device
    require_hip(store.data if store.packing is None else store.plane_params, out)
    K, C, N = int(ptr.numel()) - 1, int(cols.numel()), int(rows.numel())
    for name, t, dtype in (("ptr", ptr, torch.int64), ("rows", rows, torch.int64), ("cols", cols, torch.int32)):
        if t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"clim_seeps: {name} must be a contiguous 1-D {dtype} tensor on {dev}")
    if K < 0:
        raise ValueError("clim_seeps: ptr needs K + 1 entries")
    dry, wet_level = _dry_threshold("clim_seeps", dry), _wet_level("clim_seeps", wet_level)
    longest = max_quantile_entries()
    max_entries = longest if max_entries is None else int(max_entries)
    if not 0 <= max_entries <= longest:
        raise ValueError(f"clim_seeps: max_entries must lie in [0, {longest}], got {max_entries}")
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError(f"clim_seeps: min_count must be an integer >= 1, got {min_count!r}")
    if out is None:
        out = torch.empty(2, K, C, H, W, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (2, K, C, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"clim_seeps: out must be contiguous float32 {(2, K, C, H, W)} on {dev}")
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tail = (T, F, H, W, dptr(ptr), dptr(rows), N, K, max_entries, dptr(cols), C, dry, wet_level, int(min_count),
            dptr(out), dptr(flag), stream_ptr())
    P = H * W
    if store.packing is None:
        _lib.call("clim_seeps", 4.0 * N * C * P + 8.0 * K * C * P, dptr(store.data), *tail)
    else:
        _lib.call("clim_seeps_packed", 2.0 * N * C * P + 8.0 * K * C * P, dptr(store.codes), dptr(store.plane_params),
                  dptr(store.domain_dev), *tail)
    return out, flag


class SeepsClimatology:
    """What ``build_seeps`` returns.  ``data``: ``[2, K, C, H, W]`` float32 on the store's device, compact over the
    chosen ``names``; ``p1`` = ``data[0]``: the fraction of a cell's values below ``dry_threshold`` (NaN where a cell
    kept fewer than ``min_count`` values); ``threshold`` = ``data[1]``: the ``wet_level`` quantile of the cell's other
    values, the light / heavy edge (NaN also where there is no such value); ``plan``, ``names``, ``dry_threshold`` (as
    the float32 the kernel compared with), ``wet_level``, ``min_count``.  ``index(times_us)``: as
    ``Climatology.index``.  ``seeps.SeepsTable`` takes it as ``climatology=`` and reads ``data`` in place."""

    def __init__(self, data: torch.Tensor, plan: ClimPlan, names, dry_threshold: float, wet_level: float = 2.0 / 3.0,
                 min_count: int = 1):
        if not isinstance(data, torch.Tensor) or data.dim() != 5 or data.shape[0] != 2 or data.dtype != torch.float32:
            raise ValueError("SeepsClimatology: data must be a float32 [2, K, C, H, W] tensor")
        self.data, self.plan, self.names = data, plan, [str(n) for n in names]
        if len(self.names) != data.shape[2]:
            raise ValueError(f"SeepsClimatology: {len(self.names)} names for {data.shape[2]} channels")
        self.dry_threshold = _dry_threshold("SeepsClimatology", dry_threshold)
        self.wet_level, self.min_count = float(wet_level), int(min_count)

    @property
    def p1(self) -> torch.Tensor:
        return self.data[0]

    @property
    def threshold(self) -> torch.Tensor:
        return self.data[1]

    def index(self, times_us) -> torch.Tensor:
        return torch.from_numpy(self.plan.slot_of(times_us)).to(self.data.device)


def build_seeps(store, plan: ClimPlan, names: Sequence[str], dry_threshold, *, wet_level: float = 2.0 / 3.0,
                min_count: int = 1) -> SeepsClimatology:
    """The SEEPS climatology of ``store`` (a ``dataset.DeviceStore`` on the HIP device, float32 or packed; never written)
    by ``plan``, for the channels ``names`` (precipitation accumulations, as the store holds them), in physical units.

    Definition (the project's OWN restatement of Rodwell et al. 2010, in the spirit of WeatherBench-2; not pinned against
    any package).  For slot ``k``, channel ``c`` and cell ``p``: the values of ``build_quantiles`` - the slot's list
    entries, UNWEIGHTED, ``-0.0`` read as ``+0.0``, NaN and +-Inf skipped -, ``m`` of them kept, ``v[0] <= ... <=
    v[m-1]``.  With ``dry`` = ``float32(dry_threshold)``::

        n_dry = #{ v[i] < dry }  (strict);   n_wet = m - n_dry
        p1  = float32(n_dry / m)                                                  NaN when m < min_count
        pos = wet_level * (n_wet - 1);  lo = floor(pos);  hi = min(lo + 1, n_wet - 1);  frac = pos - lo
        thr = float32(v[n_dry+lo] + (v[n_dry+hi] - v[n_dry+lo]) * frac)           in double, one rounding;
                                                                                  NaN when n_wet < 1 or m < min_count

    ``wet_level = 2/3`` splits the wet values into "light" (two thirds) and "heavy" (one third), the categories of
    SEEPS.  One launch of ``paradis_clim_seeps`` (``csrc/quantile.hip``: ``clim_quantile``'s fill and sort, another
    stage behind them; bit-identical run to run) and one read of the launch's flag word.  Refused: what
    ``build_quantiles`` refuses - a CPU store, a plan made for other times, a plan with ``weights="gaussian"``, a name
    the store does not hold, a slot whose list is longer than ``max_quantile_entries()`` -, a ``dry_threshold`` that is
    not finite and a ``wet_level`` outside [0, 1]."""
    who = "climatology.build_seeps"
    names = [str(n) for n in ([names] if isinstance(names, str) else names)]
    if len(names) < 1:
        raise ValueError(f"{who}: names must list at least one channel")
    if plan.weights != "boxcar":
        raise ValueError(f"{who}: the plan has weights='{plan.weights}', but the SEEPS climatology is unweighted: make "
                         f"the plan with weights='boxcar'")
    dry, wet_level = _dry_threshold(who, dry_threshold), _wet_level(who, wet_level)
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError(f"{who}: min_count must be an integer >= 1, got {min_count!r}")
    if not np.array_equal(plan.times_us, store.times_us.numpy()):
        raise ValueError(f"{who}: the plan was made for other times than the store's times_us")
    column = {name: j for j, name in enumerate(store.features)}
    for name in names:
        if name not in column:
            raise ValueError(f"{who}: channel '{name}' is not among the store's features")
    longest = int(plan.entries.max()) if plan.entries.size else 0
    if longest > max_quantile_entries():
        k = int(np.argmax(plan.entries))
        raise ValueError(f"{who}: slot {k} (day of year {plan.days[k // len(plan.hours)]}, hour "
                         f"{plan.hours[k % len(plan.hours)]}) has {longest} entries, at most {max_quantile_entries()} "
                         f"can be sorted per cell: a shorter window or fewer years")
    if torch.device(store.device).type == "cpu":
        raise ValueError(f"{who}: the SEEPS climatology is built on the HIP device (no CPU fallback); got a CPU store")
    dev = store.device
    ptr, rows, _ = plan.lists()
    ptr, rows = torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev)
    cols = torch.tensor([column[n] for n in names], dtype=torch.int32, device=dev)
    data, flag = clim_seeps(store, ptr, rows, cols, dry, wet_level=wet_level, max_entries=longest,
                            min_count=int(min_count))
    if int(flag.item()):
        raise RuntimeError(f"{who}: a list entry fell outside the store (clamped by the kernel)")
    return SeepsClimatology(data, plan, names, dry, wet_level, int(min_count))
