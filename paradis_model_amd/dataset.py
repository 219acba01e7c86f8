"""A device-resident dataset: the reference's ``ERA5Dataset`` (``data/era5_dataset.py``) with the store held in HBM
(its ``training.dataset.preload: true``, the memory being the GPU's) and the batch tuple assembled by one HIP launch
for input and target (``csrc/feed.hip::paradis_assemble_batch``) plus the forcings launch of ``feed.compute_forcings``.

No dataloader workers, no pinned staging, no host-to-device copy beyond the B sample indices - and none at all when the
indices already live on the device (``DeviceLoader``), in which case ``DeviceDataset.batch`` makes no host sync and can
be captured in a HIP graph.

Restated from the reference: the feature bookkeeping of ``ERA5Dataset.__init__`` (``:97-137,150-170,266-318``), the item
of ``_getitem_standard`` / ``_getitem_prediction`` (``:337-423``) and the tables of ``_prepare_normalization``
(``:458-544``).  Reading zarr / xarray is out of scope: the store arrives as an array the user has already read.

``DeviceStore(packing="u16")`` holds the store as 16-bit codes with a float32 reference value and step per (time,
feature) plane - half the bytes - packed slab by slab on the device (``paradis_pack_planes``) and decoded inside the same
assembly launch (``paradis_assemble_batch_packed``); ``assemble_planes`` is the one place that chooses the entry point.

No CPU fallback: ``batch()`` needs the store on the HIP device.  A store built with ``device="cpu"`` serves the host
bookkeeping only (names, counts, tables, lengths).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import feed
from ._lib import check, dptr, lib, require_hip, stream_ptr
from .config import feature_layout
from .feed import KIND_HUMIDITY, KIND_PRECIP, times_to_us

EPS_Q = 1e-12                       # era5_dataset.py:58
SLAB_BYTES = 256 << 20              # host-to-device upload granularity of DeviceStore
# one row of paradis_plane_t (include/paradis_hip.h)
PLANE_DTYPE = np.dtype([("feature", "<i4"), ("dt", "<i4"), ("kind", "<i4"), ("p0", "<f4"), ("p1", "<f4")])
# the packed store (include/paradis_hip.h, "The 16-bit packed store"): per-feature domain of the packed quantity
DOMAIN_LINEAR, DOMAIN_LOG = 0, 1
PACK_MISSING = 65535


def pack_planes(slab: torch.Tensor, row0: int, codes: torch.Tensor, params: torch.Tensor, domain: torch.Tensor,
                ws_cache: Optional[dict] = None) -> None:
    """``paradis_pack_planes``: the float32 slab ``[n, F, H, W]`` into rows ``[row0, row0 + n)`` of ``codes``
    ``[T, F, H, W]`` (16-bit) and ``params`` ``[T, F, 2]``; ``domain``: device int32 ``[F]``."""
    from ._tables import workspace
    require_hip(slab, params)
    n, F, H, W = (int(v) for v in slab.shape)
    T = int(codes.shape[0])
    if tuple(codes.shape[1:]) != (F, H, W) or tuple(params.shape) != (T, F, 2) or domain.numel() != F:
        raise ValueError("pack_planes: slab, codes, params and domain disagree in shape")
    if codes.element_size() != 2 or domain.dtype != torch.int32 or not codes.is_cuda or not domain.is_cuda:
        raise ValueError("pack_planes: codes must be 16-bit and domain int32, both on the device")
    if not (slab.is_contiguous() and codes.is_contiguous() and params.is_contiguous()):
        raise ValueError("pack_planes: slab, codes and params must be contiguous")
    ws = workspace({} if ws_cache is None else ws_cache, slab.device, lib.paradis_pack_planes_ws_bytes(n, F, H, W))
    check(lib.paradis_pack_planes(dptr(slab), n, F, H, W, dptr(domain), int(row0), T, dptr(codes), dptr(params),
                                  dptr(ws), stream_ptr()), "pack_planes")


def unpack_planes(codes: torch.Tensor, params: torch.Tensor, domain: torch.Tensor, a: int, b: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``paradis_unpack_planes``: rows ``[a, b)`` of a packed store as float32 ``[b - a, F, H, W]``"""
    T, F, H, W = (int(v) for v in codes.shape)
    a, b = int(a), int(b)
    if not 0 <= a <= b <= T:
        raise IndexError(f"unpack_planes: rows [{a}, {b}) outside a store of {T}")
    if out is None:
        out = torch.empty(b - a, F, H, W, dtype=torch.float32, device=codes.device)
    require_hip(out, params)
    if tuple(out.shape) != (b - a, F, H, W) or not out.is_contiguous():
        raise ValueError(f"unpack_planes: out must be contiguous [{b - a}, {F}, {H}, {W}]")
    check(lib.paradis_unpack_planes(dptr(codes), dptr(params), dptr(domain), T, F, H, W, a, b, dptr(out), stream_ptr()),
          "unpack_planes")
    return out


def assemble_planes(store: "DeviceStore", idx: torch.Tensor, base: int, interval_steps: int, planes: torch.Tensor,
                    n_time_inputs: int, Fin: int, S: int, Fout: int, inp: torch.Tensor, tgt: Optional[torch.Tensor],
                    flag: torch.Tensor) -> None:
    """The batch-assembly launch over whatever the store holds: ``paradis_assemble_batch`` for a float32 store,
    ``paradis_assemble_batch_packed`` for a packed one - the one place that chooses."""
    T, F, H, W = store.shape
    require_hip(store.data if store.packing is None else store.plane_params, inp, tgt)
    tail = (T, F, H, W, dptr(idx), int(idx.numel()), int(base), int(interval_steps), dptr(planes), n_time_inputs, Fin, S,
            Fout, dptr(inp), dptr(tgt), EPS_Q, dptr(flag), stream_ptr())
    if store.packing is None:
        check(lib.paradis_assemble_batch(dptr(store.data), *tail), "assemble_batch")
    else:
        check(lib.paradis_assemble_batch_packed(dptr(store.codes), dptr(store.plane_params), dptr(store.domain_dev),
                                                *tail), "assemble_batch_packed")


def _hours(text) -> int:
    """"6h" -> 6 (era5_dataset.py:102,108,112)"""
    return int(str(text)[:-1])


class DeviceStore:
    """The pre-processed ERA5 store in device memory.

    data: [T, F, H, W] float32 (numpy array, memmap or tensor), the on-disk layout ``time, features, latitude,
    longitude``; uploaded in time slabs, so a memmap never needs a second full host copy.  times: [T] datetime64 or int64
    microseconds, ascending.  features: the F names.  stats: dict of [F] arrays ``mean / std / min / max`` (the
    reference's ``stats`` store), or None: computed from the uploaded data (``prepare.store_statistics``).  lat_deg [H]
    ascending, lon_deg [W].  constants: the [H, W, Cc] tensor the reference's dataset precomputes (``:193-251``).
    toa_mean / toa_std: ``toa_radiation_mean / _std`` of the stats store, or None: computed from ``times`` and the grid
    (``prepare.toa_radiation_stats``).  Computing either needs the HIP device.

    packing: None - ``data`` is the float32 store - or "u16": the store is held as 16-bit codes ``codes`` [T, F, H, W]
    with a ``(lo, step)`` pair per (time, feature) plane in ``plane_params`` [T, F, 2] (GRIB simple packing, half the
    bytes; DESIGN.md "The packed store"), ``data`` is None, and batches are decoded inside the assembly launch.
    log_packed: base names (``_h<level>`` stripped) of the features packed as ``log(x + 1e-6)``; ``domain`` [F] says
    which.  NaN and +-Inf are stored as "missing" and come back as NaN.  Each uploaded slab passes through one float32
    staging buffer of ``SLAB_BYTES``; with ``stats=None`` the statistics are taken from that slab before it is packed,
    so from the original values.  ``rows(a, b)`` gives physical float32 values of either kind of store."""

    def __init__(self, data, times, features: Sequence[str], stats, lat_deg, lon_deg, constants, toa_mean=None,
                 toa_std=None, device="cuda", packing=None, log_packed=("total_precipitation_6hr",)):
        if packing not in (None, "u16"):
            raise ValueError(f"DeviceStore: packing must be None or 'u16', got {packing!r}")
        if packing is not None and torch.device(device).type == "cpu":
            raise ValueError("DeviceStore: a packed store is packed and read on the HIP device (no CPU fallback)")
        if len(data.shape) != 4:
            raise ValueError(f"DeviceStore: data must be [T, F, H, W], got {tuple(data.shape)}")
        T, F, H, W = (int(v) for v in data.shape)
        dtype = data.dtype if isinstance(data, torch.Tensor) else torch.from_numpy(np.empty(0, data.dtype)).dtype
        if dtype != torch.float32:
            raise ValueError(f"DeviceStore: data must be float32, got {data.dtype}")
        self.features = [str(f) for f in features]
        if len(self.features) != F:
            raise ValueError(f"DeviceStore: {len(self.features)} feature names for {F} stored features")
        if len(set(self.features)) != F:
            raise ValueError("DeviceStore: feature names must be unique")
        self.times_us = times_to_us(times).contiguous()                  # host copy: date arithmetic
        if self.times_us.numel() != T:
            raise ValueError(f"DeviceStore: {self.times_us.numel()} times for {T} stored time rows")
        if T > 1 and not bool((self.times_us[1:] > self.times_us[:-1]).all()):
            raise ValueError("DeviceStore: times must be strictly ascending")
        lat = lat_deg if isinstance(lat_deg, torch.Tensor) else torch.as_tensor(np.asarray(lat_deg))
        lon = lon_deg if isinstance(lon_deg, torch.Tensor) else torch.as_tensor(np.asarray(lon_deg))
        if lat.numel() != H or lon.numel() != W:
            raise ValueError(f"DeviceStore: grid {lat.numel()}x{lon.numel()} does not match data {H}x{W}")
        if H > 1 and not bool((lat[1:] > lat[:-1]).all()):
            # the reference sorts (era5_dataset.py:77-78); flipping 48 GB silently is not this class's business
            raise ValueError("DeviceStore: latitude must be ascending (sort the store's latitude axis first)")
        if torch.device(device).type == "cpu" and (stats is None or toa_mean is None or toa_std is None):
            raise ValueError("DeviceStore: statistics need the HIP device (stats=None / toa_mean=None / toa_std=None "
                             "compute them there; this package has no CPU fallback)")
        self.stats = {}
        for key in ("mean", "std", "min", "max") if stats is not None else ():
            v = np.asarray(stats[key], dtype=np.float32).reshape(-1)      # float32 as era5_dataset.py:505-513
            if v.size != F:
                raise ValueError(f"DeviceStore: stats['{key}'] has {v.size} entries for {F} features")
            self.stats[key] = v
        # the device as tensors report it ("cuda" -> "cuda:0"): out= tensors and device indices are compared with it
        self.device = torch.empty(0, device=device).device
        self.shape = (T, F, H, W)
        self.lat, self.lon = lat.cpu(), lon.cpu()
        self.lat_dev, self.lon_dev = lat.to(self.device), lon.to(self.device)
        if toa_mean is None or toa_std is None:
            from .prepare import toa_radiation_stats
            mean, std = toa_radiation_stats(self.times_us, lat, lon, device=self.device)
            toa_mean = mean if toa_mean is None else toa_mean
            toa_std = std if toa_std is None else toa_std
        self.toa_mean, self.toa_std = float(toa_mean), float(toa_std)
        const = constants if isinstance(constants, torch.Tensor) else torch.as_tensor(np.asarray(constants))
        if const.dim() != 3 or tuple(const.shape[:2]) != (H, W):
            raise ValueError(f"DeviceStore: constants must be [H, W, Cc], got {tuple(const.shape)}")
        self.constants = const.to(device=self.device, dtype=torch.float32).contiguous()
        self.times_dev = self.times_us.to(self.device)
        self.packing = packing
        log_names = {str(n) for n in log_packed}
        self.domain = np.array([DOMAIN_LOG if packing is not None and feed.base_name(f) in log_names else DOMAIN_LINEAR
                                for f in self.features], dtype=np.int32)
        rows = max(1, SLAB_BYTES // max(1, F * H * W * 4))
        if packing is None:
            self.codes = self.plane_params = self.domain_dev = None
            self.data = torch.empty(T, F, H, W, dtype=torch.float32, device=self.device)
            for a in range(0, T, rows):
                self.data[a:a + rows].copy_(self._host_slab(data, a, rows))
            if stats is None:
                from .prepare import store_statistics
                res = store_statistics(self.data)
                self.stats = {key: res[key] for key in ("mean", "std", "min", "max")}
        else:
            from .prepare import StoreStats
            self.data = None
            self.domain_dev = torch.from_numpy(self.domain).to(self.device)
            self.codes = torch.empty(T, F, H, W, dtype=torch.uint16, device=self.device)
            self.plane_params = torch.empty(T, F, 2, dtype=torch.float32, device=self.device)
            staging = torch.empty(min(rows, T), F, H, W, dtype=torch.float32, device=self.device)
            acc = StoreStats(F, H, W, device=self.device) if stats is None else None
            ws = {}
            for a in range(0, T, rows):
                slab = self._host_slab(data, a, rows)
                on_dev = staging[:slab.shape[0]].copy_(slab)
                if acc is not None:
                    acc.update(on_dev)
                pack_planes(on_dev, a, self.codes, self.plane_params, self.domain_dev, ws)
            if acc is not None:
                res = acc.result()
                self.stats = {key: res[key] for key in ("mean", "std", "min", "max")}

    @staticmethod
    def _host_slab(data, a, rows):
        slab = data[a:a + rows]
        if not isinstance(slab, torch.Tensor):
            slab = torch.from_numpy(np.ascontiguousarray(slab))
        return slab

    @property
    def nbytes(self) -> int:
        """device bytes of the stored fields (codes and plane parameters, or the float32 array)"""
        if self.packing is None:
            return self.data.numel() * 4
        return self.codes.numel() * 2 + self.plane_params.numel() * 4

    def rows(self, a: int, b: int) -> torch.Tensor:
        """time rows ``[a, b)`` in physical units, float32 ``[b - a, F, H, W]``: a view of a float32 store, a decoded
        copy (``paradis_unpack_planes``) of a packed one"""
        T = self.shape[0]
        a, b = int(a), int(b)
        if not 0 <= a <= b <= T:
            raise IndexError(f"DeviceStore.rows: rows [{a}, {b}) outside a store of {T}")
        if self.packing is None:
            return self.data[a:b]
        return unpack_planes(self.codes, self.plane_params, self.domain_dev, a, b)

    def row_of(self, when_us: int, side: str = "left") -> int:
        """first store row at or after (``left``) / after (``right``) the given time"""
        return int(np.searchsorted(self.times_us.numpy(), when_us, side=side))


def _date_us(text: str, default_clock: str) -> int:
    text = str(text)
    if "T" not in text:
        text += default_clock                                             # era5_dataset.py:98-99,124-125
    return int(np.datetime64(text, "us").astype(np.int64))


class DeviceDataset:
    """``ERA5Dataset(..., preload=True)`` over a ``DeviceStore``: the same samples, ``batch(indices)`` instead of
    ``__getitem__`` + collate.  Exposes what ``Paradis.__init__`` and the trainer read from the reference's dataset /
    datamodule (``num_in_features``, ``num_out_features``, ``num_common_features``, ``output_name_order``, ``lat``,
    ``lon``, ``lat_size``, ``lon_size``, and itself as ``.dataset``), so it can stand where ``stub_datamodule(cfg)``
    stands.

    cfg keys read: ``features.*``, ``dataset.n_time_inputs``, ``dataset.time_resolution`` / ``sampling_interval`` /
    ``prediction_delta`` (default "6h" each, the shipped values) and ``normalization.standard`` (default False, shipped).
    """

    def __init__(self, store: DeviceStore, cfg, start_date: str, end_date: Optional[str], forecast_steps: int,
                 prediction_stage: bool = False):
        self.store, self.cfg = store, cfg
        self.forecast_steps = S = int(forecast_steps)
        self.prediction_stage = bool(prediction_stage)
        if S < 1:
            raise ValueError(f"DeviceDataset: forecast_steps={S} must be >= 1")
        ds_cfg = cfg.dataset
        self.n_time_inputs = n_t = int(ds_cfg.n_time_inputs) if int(ds_cfg.n_time_inputs) > 1 else 1
        self.time_resolution = res = _hours(ds_cfg.get("time_resolution", "6h"))
        interval = ds_cfg.get("sampling_interval", None)
        self.interval_steps = (res if interval is None else _hours(interval)) // res
        if self.interval_steps < 1:
            raise ValueError("DeviceDataset: dataset.sampling_interval is shorter than dataset.time_resolution")
        self.prediction_shift = (_hours(ds_cfg.get("prediction_delta", "6h")) // res - 1) * self.interval_steps
        norm_cfg = cfg.get("normalization", None)
        self.custom_normalization = not bool(norm_cfg.get("standard", False)) if norm_cfg is not None else True
        self.forcing_inputs = list(cfg.features.input.forcings)

        # ---- features: common first, then input-only / output-only (era5_dataset.py:150-166,266-279)
        levels = list(cfg.features.pressure_levels)
        in_feats = [f"{v}_h{l}" for v in cfg.features.input.atmospheric for l in levels] + list(cfg.features.input.surface)
        out_feats = ([f"{v}_h{l}" for v in cfg.features.output.atmospheric for l in levels]
                     + list(cfg.features.output.surface))
        common = [f for f in out_feats if f in in_feats]
        self.dyn_input_features = common + [f for f in in_feats if f not in out_feats]
        self.dyn_output_features = common + [f for f in out_feats if f not in in_feats]
        Fin, Fout = len(self.dyn_input_features), len(self.dyn_output_features)
        column = {name: j for j, name in enumerate(store.features)}
        for name in self.dyn_input_features + self.dyn_output_features:
            if name not in column:
                raise ValueError(f"DeviceDataset: configured feature '{name}' is not in the store")
        self.in_columns = [column[f] for f in self.dyn_input_features]
        self.out_columns = [column[f] for f in self.dyn_output_features]
        lay = feature_layout(cfg)
        self.num_common_features = len(common)
        self.num_dyn_inputs_single = Fin
        self.num_in_dyn_features = Fin * n_t + len(self.forcing_inputs) * n_t
        self.num_in_static_features = int(store.constants.shape[-1])
        self.num_in_features = self.num_in_dyn_features + self.num_in_static_features
        self.num_out_features = Fout
        self.output_name_order = list(self.dyn_output_features)
        if (lay.num_common_features, lay.num_out_features, lay.dyn_single, lay.num_in_dyn_features) != \
                (self.num_common_features, Fout, Fin, self.num_in_dyn_features) or \
                lay.output_name_order != self.output_name_order:
            raise ValueError("DeviceDataset: config.feature_layout disagrees with the dataset's feature bookkeeping")
        self.dataset = self                          # the datamodule's ``.dataset`` (model/paradis.py reads it)
        self.lat, self.lon = store.lat, store.lon
        self.lat_size, self.lon_size = store.shape[2], store.shape[3]

        # ---- time bookkeeping (era5_dataset.py:97-137)
        T = store.shape[0]
        start_us = _date_us(start_date, "T00:00:00")
        first_us = start_us - (n_t - 1) * res * 3600 * 1000000
        if first_us < int(store.times_us[0]):
            raise ValueError(f"DeviceDataset: the inputs of the first sample ({n_t} times ending at {start_date}) start "
                             "before the store does")
        self.base = store.row_of(first_us, "left")
        lo = store.row_of(start_us, "left")
        hi = T if end_date is None else store.row_of(_date_us(end_date, "T23:59:59"), "right")
        self.length = len(range(lo, hi, self.interval_steps))            # ds.sel(time=slice(start, end, interval))
        self.time = store.times_us[lo:hi:self.interval_steps].numpy().astype("datetime64[us]")
        self.n_forcing_times = S + n_t - 1
        if self.length > 0:
            t_in = self.base + (self.length - 1) * self.interval_steps
            if t_in + self.n_forcing_times > T:
                raise ValueError(f"DeviceDataset: the inputs of the last sample (index {self.length - 1}) need store "
                                 f"row {t_in + self.n_forcing_times - 1}, the store has {T}")
            last_target = t_in + n_t + self.prediction_shift + S - 1
            if not self.prediction_stage and last_target >= T:
                raise ValueError(f"DeviceDataset: the targets of the last sample (index {self.length - 1}) need store "
                                 f"row {last_target}, the store has {T}")

        # ---- normalisation tables (era5_dataset.py:458-544) and the plane table of the kernel
        st = store.stats
        kinds_in = [self._kind_of(f) for f in self.dyn_input_features]
        hum_cols = [c for c, k in zip(self.in_columns, kinds_in) if k == KIND_HUMIDITY]
        if hum_cols:                                    # :528-537, float32 like the reference's tensors
            self.q_max = np.float32(st["max"][hum_cols].max())
            self.q_min = np.float32(st["min"][hum_cols].min())
            if self.q_min < EPS_Q:
                self.q_min = np.float32(EPS_Q)
        else:                                           # :539-540
            self.q_max, self.q_min = np.float32(0.0), np.float32(EPS_Q)
        self.kind_in, self.p0_in, self.p1_in = self._tables(self.dyn_input_features, self.in_columns)
        self.kind_out, self.p0_out, self.p1_out = self._tables(self.dyn_output_features, self.out_columns)
        table = np.zeros(n_t * Fin + S * Fout, dtype=PLANE_DTYPE)
        for k in range(n_t):                            # input channel k*Fin + j: time t_in + k (:362-366)
            rows = table[k * Fin:(k + 1) * Fin]
            rows["feature"], rows["dt"] = self.in_columns, k
            rows["kind"], rows["p0"], rows["p1"] = self.kind_in, self.p0_in, self.p1_in
        for s in range(S):                              # target step s: time t_in + n_t + shift + s (:351-354)
            rows = table[n_t * Fin + s * Fout:n_t * Fin + (s + 1) * Fout]
            rows["feature"], rows["dt"] = self.out_columns, n_t + self.prediction_shift + s
            rows["kind"], rows["p0"], rows["p1"] = self.kind_out, self.p0_out, self.p1_out
        self.plane_table = table
        dev = store.device
        self._planes = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        self._flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._offsets = torch.arange(self.n_forcing_times, dtype=torch.int64, device=dev)
        self._constants = {}

    # ------------------------------------------------------------------ tables
    def _kind_of(self, feature: str) -> int:
        return feed.kind_of(feature, self.custom_normalization)

    def _tables(self, names, columns):
        st = self.store.stats
        kind = np.array([self._kind_of(f) for f in names], dtype=np.int32)
        p0 = st["mean"][columns].astype(np.float32)
        p1 = st["std"][columns].astype(np.float32)
        p0[kind == KIND_HUMIDITY], p1[kind == KIND_HUMIDITY] = self.q_min, self.q_max
        p0[kind == KIND_PRECIP], p1[kind == KIND_PRECIP] = 0.0, 0.0
        return kind, p0, p1

    def __len__(self) -> int:
        return self.length

    # ------------------------------------------------------------------ batches
    def batch_shapes(self, B: int):
        """shapes of (input, target, forcings, constants) for B samples"""
        _, _, H, W = self.store.shape
        S, n_t = self.forecast_steps, self.n_time_inputs
        n_forc = len([v for v in self.forcing_inputs if v in feed.FORCING_CODES]) * n_t
        return ((B, 1, n_t * self.num_dyn_inputs_single, H, W), (B, S, self.num_out_features, H, W),
                (B, S, H, W, n_forc), (B, 1, H, W, self.num_in_static_features))

    def _indices(self, indices) -> torch.Tensor:
        dev = self.store.device
        if isinstance(indices, torch.Tensor) and indices.device.type != "cpu":
            if indices.dtype != torch.int64 or indices.dim() != 1 or indices.device != dev:
                raise ValueError("DeviceDataset.batch: device indices must be a 1-D int64 tensor on the store's device")
            return indices.contiguous()
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.length):
            raise IndexError(f"DeviceDataset.batch: sample index outside [0, {self.length})")
        return idx.to(dev)

    def _constants_for(self, B: int) -> torch.Tensor:
        c = self._constants.get(B)
        if c is None:
            H, W, Cc = self.store.constants.shape
            c = self._constants[B] = self.store.constants.view(1, 1, H, W, Cc).expand(B, 1, H, W, Cc).contiguous()
        return c

    def _check_out(self, out, shapes):
        if len(out) != len(shapes):
            raise ValueError(f"DeviceDataset.batch: out= needs {len(shapes)} tensors, got {len(out)}")
        for name, t, shape in zip(self._out_names(), out, shapes):
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"DeviceDataset.batch: out {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"DeviceDataset.batch: out {name} must be float32, got {t.dtype}")
            if t.device != self.store.device:
                raise ValueError(f"DeviceDataset.batch: out {name} is on {t.device}, the store on {self.store.device}")
            if not t.is_contiguous():
                raise ValueError(f"DeviceDataset.batch: out {name} must be contiguous")

    def _out_names(self):
        return ("input", "forcings", "constants") if self.prediction_stage else ("input", "target", "forcings", "constants")

    def assemble(self, idx: torch.Tensor, inp: torch.Tensor, tgt: Optional[torch.Tensor]) -> None:
        """The one launch: input and (unless ``tgt`` is None) target of the samples ``idx`` (device int64) into the given
        contiguous float32 tensors.  No checks beyond the C entry point's: ``batch`` is the public way in."""
        assemble_planes(self.store, idx, self.base, self.interval_steps, self._planes, self.n_time_inputs,
                        self.num_dyn_inputs_single, self.forecast_steps, self.num_out_features, inp, tgt, self._flag)

    def batch(self, indices, out=None):
        """(input [B,1,n_t*Fin,H,W], target [B,S,Fout,H,W], forcings [B,S,H,W,Nf], constants [B,1,H,W,Cc]) of the samples
        ``indices``: contiguous float32 on the device, what ``harness.rollout_loss`` consumes (reference
        ``_getitem_standard`` + collate).  With ``prediction_stage`` the tuple is (indices, input, forcings, constants),
        as ``_getitem_prediction``.

        indices: a Python sequence or CPU tensor is range-checked on the host (``IndexError``) and copied once; a device
        int64 tensor is used as it is - no host sync, capturable; an index outside the store then reads clamped time rows
        and raises the flag of ``index_errors()``.  out: the tensors to write into, in the order they are returned
        (without ``indices``), e.g. ``GraphedTrainStep.static_batch``; the same tensors are returned.  The constants are
        materialised once per batch size; without ``out`` every call returns that same tensor."""
        idx = self._indices(indices)
        B = int(idx.numel())
        shapes = self.batch_shapes(B)
        if self.prediction_stage:
            shapes = (shapes[0], shapes[2], shapes[3])
        if out is not None:
            out = tuple(out)
            self._check_out(out, shapes)
        dev = self.store.device
        inp = out[0] if out is not None else torch.empty(shapes[0], dtype=torch.float32, device=dev)
        tgt = None
        if not self.prediction_stage:
            tgt = out[1] if out is not None else torch.empty(shapes[1], dtype=torch.float32, device=dev)
        forc_out, const_out = (out[-2], out[-1]) if out is not None else (None, None)
        if B > 0:
            T = self.store.shape[0]
            self.assemble(idx, inp, tgt)
            # times of each sample's forcing window, gathered on the device (rows clamped like the kernel's)
            rows = (self.base + idx * self.interval_steps).unsqueeze(1) + self._offsets
            times = self.store.times_dev[rows.clamp_(0, T - 1)]
            forc = feed.compute_forcings(times, self.store.lat_dev, self.store.lon_dev, self.n_time_inputs,
                                         self.store.toa_mean, self.store.toa_std, self.forcing_inputs, device=dev)
            if forc_out is not None and forc is not None:
                forc = forc_out.copy_(forc)
            const = self._constants_for(B)
            if const_out is not None:
                const = const_out.copy_(const)
        else:
            forc = forc_out if forc_out is not None else torch.empty(shapes[-2], dtype=torch.float32, device=dev)
            const = const_out if const_out is not None else torch.empty(shapes[-1], dtype=torch.float32, device=dev)
        if self.prediction_stage:
            return idx, inp, forc, const
        return inp, tgt, forc, const

    def index_errors(self, clear: bool = False) -> int:
        """Non-zero when a batch since construction (or the last ``clear``) had an index whose times fall outside the
        store (possible with device indices only).  Reads one device word: the only sync of this class, and the caller
        chooses when."""
        v = int(self._flag.item())
        if clear:
            self._flag.zero_()
        return v


def epoch_indices(n: int, epoch: int = 0, shuffle: bool = False, seed: int = 0, rank: int = 0,
                  world_size: int = 1) -> torch.Tensor:
    """The sample indices of one rank for one epoch (CPU int64): a permutation from a CPU generator seeded with
    ``seed + epoch`` (or 0..n-1), padded by wrapping to a multiple of ``world_size`` and strided ``rank::world_size`` -
    the rule of ``torch.utils.data.DistributedSampler``."""
    if not 0 <= rank < world_size:
        raise ValueError(f"epoch_indices: rank {rank} outside [0, {world_size})")
    if shuffle:
        g = torch.Generator().manual_seed(int(seed) + int(epoch))
        perm = torch.randperm(n, generator=g)
    else:
        perm = torch.arange(n, dtype=torch.int64)
    if world_size > 1 and n > 0:
        total = -(-n // world_size) * world_size
        while perm.numel() < total:
            perm = torch.cat([perm, perm[:total - perm.numel()]])
        perm = perm[rank:total:world_size]
    return perm.contiguous()


def batch_bounds(n: int, batch_size: int, drop_last: bool):
    """[(begin, end)] of the batches over n indices"""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    stop = (n // batch_size) * batch_size if drop_last else n
    return [(a, min(a + batch_size, stop)) for a in range(0, stop, batch_size)]


class DeviceLoader:
    """Iterates ``dataset.batch`` over an epoch: the epoch's index vector (``epoch_indices``) is copied to the device
    once, every batch is a device slice of it - no per-batch host-to-device traffic, no sync.  ``set_epoch(e)`` as
    ``DistributedSampler``."""

    def __init__(self, dataset: DeviceDataset, batch_size: int, shuffle: bool = False, drop_last: bool = False,
                 seed: int = 0, rank: int = 0, world_size: int = 1):
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.shuffle, self.drop_last, self.seed = bool(shuffle), bool(drop_last), int(seed)
        self.rank, self.world_size, self.epoch = int(rank), int(world_size), 0
        self._bounds = batch_bounds(len(self.indices()), self.batch_size, self.drop_last)

    def indices(self) -> torch.Tensor:
        return epoch_indices(len(self.dataset), self.epoch, self.shuffle, self.seed, self.rank, self.world_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return len(self._bounds)

    def __iter__(self):
        idx = self.indices().to(self.dataset.store.device)
        for a, b in self._bounds:
            yield self.dataset.batch(idx[a:b])
