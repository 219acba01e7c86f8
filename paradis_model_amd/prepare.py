"""Store preparation on the device: what the reference's ``scripts/preprocess_dataset.py`` does between raw ERA5 fields
and the store that ``dataset.DeviceStore`` serves, without xarray / dask / zarr.

  ``cartesian_winds``       its ``compute_cartesian_wind`` (``:42-105``): every level and the 10 m winds in one launch
  ``StoreStats``            its ``compute_statistics`` (``:409-479``) and ``compute_tendency_statistics`` (``:482-590``):
                            mean / std / min / max per feature, and the same of ``x[t + stride] - x[t]``, streamed over
                            time slabs in one pass each (``csrc/prepare.hip``)
  ``toa_radiation_stats``   ``data/forcings/toa_radiation.py:203-238``, over the forcings launch of ``feed``

Reading or writing zarr, the ``BitRound(15)`` filter of the reference's stats store, ``precompute_static_data`` and
sorting the latitude axis are out of scope.  No CPU fallback: the tensors live on the HIP device.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import feed
from ._lib import check, dptr, lib, require_hip, stream_ptr
from ._tables import device_tables, trig_tables, workspace

# one row of paradis_wind_row_t (include/paradis_hip.h)
WIND_DTYPE = np.dtype([("src_u", "<i4"), ("src_v", "<i4"), ("src_w", "<i4"), ("src_t", "<i4"), ("dst_x", "<i4"),
                       ("dst_y", "<i4"), ("dst_z", "<i4"), ("level_hpa", "<f4")])
STATS_Q = 5                                  # n, sum, sum of squares, min, max (csrc/prepare.hip)
TOA_CHUNK_VALUES = 1 << 24                   # values of TOA radiation held at once by toa_radiation_stats (64 MiB)


class WindPlan:
    """The table of ``paradis_cartesian_winds``: one row per pressure level and one for the 10 m winds, built from the
    reference's feature names.  Sources ``u_component_of_wind_h{l}``, ``v_component_of_wind_h{l}``,
    ``vertical_velocity_h{l}``, ``temperature_h{l}``, ``10m_u_component_of_wind``, ``10m_v_component_of_wind`` are looked
    up in ``src_features``; destinations ``wind_x_h{l}``, ``wind_y_h{l}``, ``wind_z_h{l}``, ``wind_x_10m``,
    ``wind_y_10m``, ``wind_z_10m`` in ``dst_features``.  ``levels``: the pressure levels in hPa, as the names carry them."""

    def __init__(self, src_features: Sequence[str], dst_features: Sequence[str], levels: Sequence):
        self.src_features = [str(f) for f in src_features]
        self.dst_features = [str(f) for f in dst_features]
        self.levels = list(levels)
        src = {name: j for j, name in enumerate(self.src_features)}
        dst = {name: j for j, name in enumerate(self.dst_features)}

        def col(table, name, side):
            if name not in table:
                raise ValueError(f"WindPlan: {side} feature '{name}' is missing")
            return table[name]

        rows = np.zeros(len(self.levels) + 1, dtype=WIND_DTYPE)
        for i, l in enumerate(self.levels):
            if not float(l) > 0.0:
                raise ValueError(f"WindPlan: pressure level {l} hPa must be > 0")
            rows[i] = (col(src, f"u_component_of_wind_h{l}", "source"), col(src, f"v_component_of_wind_h{l}", "source"),
                       col(src, f"vertical_velocity_h{l}", "source"), col(src, f"temperature_h{l}", "source"),
                       col(dst, f"wind_x_h{l}", "destination"), col(dst, f"wind_y_h{l}", "destination"),
                       col(dst, f"wind_z_h{l}", "destination"), float(l))
        rows[-1] = (col(src, "10m_u_component_of_wind", "source"), col(src, "10m_v_component_of_wind", "source"), -1, -1,
                    col(dst, "wind_x_10m", "destination"), col(dst, "wind_y_10m", "destination"),
                    col(dst, "wind_z_10m", "destination"), 0.0)
        self.rows = rows
        written = [int(r[k]) for r in rows for k in ("dst_x", "dst_y", "dst_z")]
        if len(set(written)) != len(written):
            raise ValueError("WindPlan: two destinations share a column")
        # src may be dst when no destination column is a column that some row reads
        read = {int(r[k]) for r in rows for k in ("src_u", "src_v", "src_w", "src_t")} - {-1}
        self.in_place_ok = not (read & set(written))
        self._dev, self._trig = {}, {}

    def device_rows(self, device) -> torch.Tensor:
        return (self._dev.get(device) or device_tables(self._dev, device, device, (self.rows.view(np.uint8),)))[0]

    def trig_tables(self, lat_deg, lon_deg, device):
        """the double sin / cos tables of the grid on ``device``, built once (``_tables.trig_tables``)"""
        return trig_tables(self._trig, lat_deg, lon_deg, device)


def _dense4(t, name, who):
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError(f"{who}: {name} must be a [T, F, H, W] tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous float32, got {t.dtype}")


def cartesian_winds(src: torch.Tensor, dst: torch.Tensor, plan: WindPlan, lat_deg, lon_deg) -> torch.Tensor:
    """``compute_cartesian_wind`` of the reference on the device, one launch: ``dst[:, wind_*]`` from ``src[:, u, v,
    omega, T]`` for every level of ``plan`` and the 10 m winds.  src [T, Fs, H, W], dst [T, Fd, H, W] float32 on the
    device; ``dst`` may be ``src`` when the plan's destinations are none of its sources (the raw fields and the
    Cartesian winds side by side in one tensor).  Columns the plan does not name are not touched.  lat_deg [H],
    lon_deg [W]: degrees.  The float64 expression of the float32 fields, rounded once (numpy with float64 grids).
    Returns ``dst``."""
    _dense4(src, "src", "cartesian_winds")
    _dense4(dst, "dst", "cartesian_winds")
    require_hip(src, dst)
    T, Fs, H, W = src.shape
    if dst.device != src.device or (dst.shape[0], dst.shape[2], dst.shape[3]) != (T, H, W):
        raise ValueError(f"cartesian_winds: dst {tuple(dst.shape)} on {dst.device} does not match src "
                         f"{tuple(src.shape)} on {src.device}")
    Fd = dst.shape[1]
    if Fs != len(plan.src_features) or Fd != len(plan.dst_features):
        raise ValueError(f"cartesian_winds: the plan names {len(plan.src_features)} source and "
                         f"{len(plan.dst_features)} destination features, the tensors hold {Fs} and {Fd}")
    if src.untyped_storage().data_ptr() == dst.untyped_storage().data_ptr():
        if src.data_ptr() != dst.data_ptr() or src.shape != dst.shape:
            raise ValueError("cartesian_winds: src and dst overlap without being the same tensor")
        if not plan.in_place_ok:
            raise ValueError("cartesian_winds: in place, a destination column of the plan is also a source column")
    trig, th, tw = plan.trig_tables(lat_deg, lon_deg, src.device)
    if (th, tw) != (H, W):
        raise ValueError(f"cartesian_winds: lat/lon of {th} x {tw} points for {H} x {W} fields")
    rows = plan.device_rows(src.device)
    check(lib.paradis_cartesian_winds(dptr(src), Fs, dptr(dst), Fd, dptr(rows), plan.rows.ctypes.data, len(plan.rows),
                                      dptr(trig), T, H, W, stream_ptr()), "cartesian_winds")
    return dst


class StoreStats:
    """Streaming per-feature statistics of a store ``[T, F, H, W]`` fed in time slabs: the reference's
    ``compute_statistics`` and, per entry of ``strides``, ``compute_tendency_statistics`` with that stride (its
    ``delta_hours / native_dt_hours``).  NaN is skipped (``skipna=True``), ``std`` has ``ddof = 0``.

    ``update(slab)`` launches on the current stream and makes no host sync; the object keeps the last ``max(strides)``
    rows it has seen, so a tendency whose two rows fall in different slabs is counted, whatever the slab lengths.
    ``result()`` reads the accumulator once.  For a given partition into slabs the result is bit-identical run to run."""

    def __init__(self, n_features: int, H: int, W: int, strides: Sequence[int] = (), device="cuda"):
        self.F, self.H, self.W = int(n_features), int(H), int(W)
        if self.F < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"StoreStats: bad shape F={self.F} H={self.H} W={self.W}")
        self.strides = [int(s) for s in strides]
        for s in self.strides:
            if s < 1:
                raise ValueError(f"StoreStats: stride {s} must be >= 1")
        if len(set(self.strides)) != len(self.strides):
            raise ValueError("StoreStats: strides must be distinct")
        self.device = torch.device(device)
        if self.device.type == "cpu":
            raise ValueError("StoreStats: statistics need the HIP device (this package has no CPU fallback)")
        self.n_sets = 1 + len(self.strides)
        self.keep = max(self.strides, default=0)
        self.rows_seen = 0
        self._acc = self._tail = None
        self._ws = {}

    def _accumulator(self) -> torch.Tensor:
        if self._acc is None:                               # first touch of the device: construction is host-only
            init = np.zeros((self.F, self.n_sets + 1, STATS_Q))
            init[:, :self.n_sets, 3], init[:, :self.n_sets, 4] = np.inf, -np.inf
            self._acc = torch.from_numpy(init).to(self.device)
            self.device = self._acc.device
        return self._acc

    def update(self, slab) -> None:
        """the next ``[t, F, H, W]`` float32 rows of the store: a device tensor is read in place, a numpy array or CPU
        tensor is uploaded first"""
        if not isinstance(slab, torch.Tensor):
            slab = torch.from_numpy(np.ascontiguousarray(slab))
        if slab.dim() != 4 or tuple(slab.shape[1:]) != (self.F, self.H, self.W):
            raise ValueError(f"StoreStats.update: slab must be [t, {self.F}, {self.H}, {self.W}], got {tuple(slab.shape)}")
        if slab.dtype != torch.float32:
            raise ValueError(f"StoreStats.update: slab must be float32, got {slab.dtype}")
        acc = self._accumulator()
        slab = slab.to(self.device).contiguous()
        require_hip(slab)
        t = int(slab.shape[0])
        if t == 0:
            return
        ws = workspace(self._ws, self.device, lib.paradis_store_stats_ws_bytes(t, self.F, self.H, self.W))
        tail, n_prev = self._tail, 0 if self._tail is None else int(self._tail.shape[0])
        # the field with the first stride's tendency in one pass (8 B per value instead of 12), further strides alone
        passes = [(0, 1 if self.strides else -1, self.strides[0] if self.strides else 1)]
        passes += [(-1, 1 + i, s) for i, s in enumerate(self.strides) if i > 0]
        for field_set, tend_set, stride in passes:
            check(lib.paradis_store_stats(dptr(slab), t, dptr(tail), n_prev, self.F, self.H, self.W, field_set, tend_set,
                                          stride, dptr(acc), self.n_sets, dptr(ws), stream_ptr()), "store_stats")
        if self.keep:
            if t >= self.keep:
                self._tail = slab[t - self.keep:].clone()
            else:
                self._tail = torch.cat([tail, slab])[-self.keep:].contiguous() if tail is not None else slab.clone()
        self.rows_seen += t

    def _moments(self):
        """float64 (n, mean, std, min, max), each [n_sets, F]; NaN where a feature has no valid value"""
        for s in self.strides:
            if self.rows_seen < s + 1:
                raise ValueError(f"StoreStats.result: a tendency of stride {s} needs at least {s + 1} time rows, "
                                 f"{self.rows_seen} were seen")
        a = self._accumulator().cpu().numpy()                                   # the one read
        sets = a[:, :self.n_sets].transpose(1, 0, 2)                            # [n_sets, F, 5]
        n, s1, s2 = sets[..., 0], sets[..., 1], sets[..., 2]
        pivot = np.zeros_like(n)
        pivot[0] = a[:, self.n_sets, 0]                                          # tendencies are summed about 0
        with np.errstate(invalid="ignore", divide="ignore"):
            m = s1 / n
            mean = pivot + m
            std = np.sqrt(np.maximum(s2 / n - m * m, 0.0))
        empty = n == 0
        out = [np.where(empty, np.nan, v) for v in (mean, std, sets[..., 3], sets[..., 4])]
        return (n, *out)

    def result(self) -> dict:
        """``mean / std / min / max`` ([F] float32, as the reference stores them) and ``count`` ([F] int64, the non-NaN
        values) of the rows seen so far, and under ``tendencies[stride]`` the reference's ``tendency_mean / _std / _min
        / _max``, their ``count`` and ``n_samples`` (rows seen - stride).  A feature without a valid value is NaN."""
        n, mean, std, mn, mx = self._moments()
        f32 = lambda v: v.astype(np.float32)                                     # noqa: E731
        res = {"mean": f32(mean[0]), "std": f32(std[0]), "min": f32(mn[0]), "max": f32(mx[0]),
               "count": n[0].astype(np.int64), "tendencies": {}}
        for i, s in enumerate(self.strides, start=1):
            res["tendencies"][s] = {"tendency_mean": f32(mean[i]), "tendency_std": f32(std[i]),
                                    "tendency_min": f32(mn[i]), "tendency_max": f32(mx[i]),
                                    "count": n[i].astype(np.int64), "n_samples": self.rows_seen - s}
        return res


def store_statistics(data: torch.Tensor, strides: Sequence[int] = ()) -> dict:
    """``StoreStats`` over a resident ``[T, F, H, W]`` tensor in one call: the dict of ``StoreStats.result``"""
    if not isinstance(data, torch.Tensor) or data.dim() != 4:
        raise ValueError("store_statistics: data must be a [T, F, H, W] tensor on the device")
    if data.device.type == "cpu":
        raise ValueError("store_statistics: statistics need the HIP device (this package has no CPU fallback)")
    _, F, H, W = data.shape
    st = StoreStats(F, H, W, strides, device=data.device)
    st.update(data)
    return st.result()


def toa_radiation_stats(times, lat_deg, lon_deg, time_stride: int = 1, lat_stride: int = 1, lon_stride: int = 1,
                        device="cuda"):
    """The reference's ``toa_radiation_stats`` (``data/forcings/toa_radiation.py:203-238``): global (mean, std) of the 1 h
    TOA radiation over ``times[::time_stride]`` x ``lat[::lat_stride]`` x ``lon[::lon_stride]``, as Python floats - the
    ``toa_radiation_mean / _std`` of its stats store.  The radiation comes from ``feed.compute_forcings`` (TOA alone,
    mean 0, std 1) in time chunks of bounded size, each fed to a one-feature ``StoreStats``.

    Restated with it: the reference converts the latitudes to float32 radians and hands them to ``toa_radiation_1h``,
    which converts degrees to radians once more (``:221`` and ``:134``).  The stats store a trained model was
    normalised with holds the result of that, so the same values are computed here."""
    if torch.device(device).type == "cpu":
        raise ValueError("toa_radiation_stats: statistics need the HIP device (this package has no CPU fallback)")
    t_us = feed.times_to_us(times).reshape(-1)[::int(time_stride)].contiguous()
    lat, lon = (np.asarray(g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g).reshape(-1)
                for g in (lat_deg, lon_deg))
    lat, lon = lat[::int(lat_stride)], lon[::int(lon_stride)]
    lat_arg = (lat * np.pi / 180).astype(np.float32)                             # :221, read as degrees by :134
    lon_arg = lon.astype(np.float32)                                             # :222
    H, W = lat_arg.size, lon_arg.size
    st = StoreStats(1, H, W, device=device)
    lat_dev, lon_dev = torch.from_numpy(lat_arg).to(device), torch.from_numpy(lon_arg).to(device)
    rows = max(1, TOA_CHUNK_VALUES // (H * W))
    for a in range(0, t_us.numel(), rows):
        rad = feed.compute_forcings(t_us[a:a + rows], lat_dev, lon_dev, 1, 0.0, 1.0, ["toa_incident_solar_radiation"],
                                    device=device)                               # [t, H, W, 1]
        st.update(rad.view(-1, 1, H, W))
    _, mean, std, _, _ = st._moments()
    return float(mean[0, 0]), float(std[0, 0])
