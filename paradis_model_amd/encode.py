"""The writer's side of the forecast path: what the reference does to a chunk between ``predict_step`` and the bytes of
a zarr region write (``utils/file_output.py``), on the device.

``forecast.Forecaster`` hands over a physical-unit chunk ``[B, n, C, H, W]`` in model channel order plus a dew-point
chunk.  The reference's ``_build_dataset_for_samples`` (``:66-175``) regroups the channels into named variables
``[time, prediction_timedelta, level, latitude, longitude]`` by fancy indexing, renames the winds, drops ``wind_z_10m``,
prepends the initial state on the first chunk, adds ``dewpoint_depression``, and its encoding (``:18-24,262-263``) runs
every float through ``BitRound(keepbits=16)`` in front of the compressor.  Here ``csrc/encode.hip`` does the regrouping
and the rounding in one launch per flushed chunk (``encode_chunk``), into one buffer that holds every variable as a
contiguous block (``EncodeSpec.views``); ``initial_state`` builds the state of slot 0 from the device-resident store.

Host-only restatements: the renames and variable loops (``EncodeSpec.from_config``), the store template
(``EncodeSpec.template``, ``_build_template_dataset`` ``:178-279``) and the region bookkeeping of a chunk (``regions``,
``write_forecast_region_chunked`` ``:299-349``).

Out of scope: the container.  zarr, xarray, numcodecs and Blosc are not dependencies; the shuffle / zstd compressor and
the zarr metadata stay with the writer.  Two things are restated and NOT pinned against their packages, which no test
here can import: the BitRound arithmetic (numcodecs' published ``BitRound.encode``) and the renames of
``_replace_variable_names`` (the reference module needs xarray / dask to import).

No CPU fallback: ``encode_chunk`` and ``initial_state`` need the HIP device.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, lib, require_hip, stream_ptr
from ._tables import batch_stride, dense_state, device_tables
from .feed import KIND_NONE

# one row of paradis_encode_plane_t (include/paradis_hip.h)
ENCODE_PLANE_DTYPE = np.dtype([("src", "<i4"), ("first", "<i4"), ("levels", "<i4"), ("level", "<i4")])
# _replace_variable_names (utils/file_output.py:48-63); restated, unpinned (see the module docstring)
ATMOSPHERIC_RENAMES = {"wind_x": "u_component_of_wind", "wind_y": "v_component_of_wind", "wind_z": "vertical_velocity"}
SURFACE_RENAMES = {"wind_x_10m": "10m_u_component_of_wind", "wind_y_10m": "10m_v_component_of_wind"}
SKIPPED_SURFACE = ("wind_z_10m",)
DEWPOINT_NAME = "dewpoint_depression"
ATM_DIMS = ("time", "prediction_timedelta", "level", "latitude", "longitude")
SFC_DIMS = ("time", "prediction_timedelta", "latitude", "longitude")
CHUNK_TIMEDELTAS = 10           # the `min(10, total_pred_steps)` of the reference's chunking
MANTISSA_BITS = 23              # float32; numcodecs' max_bits["float32"]


def _level_tag(level) -> str:
    """``50`` and ``50.0`` both name the channel ``_h50``"""
    return str(int(level)) if float(level).is_integer() else str(level)


class Variable(NamedTuple):
    name: str
    levels: int                 # L_v: 1 for a surface variable
    surface: bool
    sources: Tuple[int, ...]    # per level: channel of the chunk (>= 0) or -1 - level of the dew-point chunk
    first: int                  # planes per (sample, time slot) of the variables in front of this one


class Region(NamedTuple):
    rows: np.ndarray            # positions in the batch of this run's samples, in ascending sample order
    time: slice                 # the run's slice of the store's sorted time axis
    prediction_timedelta: slice


@dataclass
class EncodeSpec:
    """The variables of the reference's writer for one output feature list, and the plane table of
    ``paradis_forecast_encode`` (built once; the device copy once per device)."""
    names: List[str]                     # the chunk's channel names (PostSpec.names)
    pressure_levels: List
    keepbits: Optional[int]              # 1 .. 23, or None: no rounding
    dewpoint: bool
    variables: List[Variable]
    shadowed: List[str]                  # channels a later variable of the same name replaced (not written)
    table: np.ndarray                    # [n_planes] ENCODE_PLANE_DTYPE
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def num_channels(self) -> int:
        return len(self.names)

    @property
    def num_levels(self) -> int:
        return len(self.pressure_levels)

    @property
    def n_planes(self) -> int:
        """output planes per (sample, time slot)"""
        return int(self.table.shape[0])

    @property
    def keepbits_code(self) -> int:
        """the C entry point's ``keepbits``: 0 is "off" """
        return 0 if self.keepbits is None else int(self.keepbits)

    @classmethod
    def from_config(cls, cfg, names: Sequence[str], pressure_levels: Sequence, keepbits: Optional[int] = 16,
                    dewpoint: bool = True) -> "EncodeSpec":
        """``_replace_variable_names`` and the variable loops of ``_build_dataset_for_samples`` for the chunk whose
        channels are ``names``.  Two outputs that share a name after the renames (the shipped config lists both
        ``wind_z`` and ``vertical_velocity``) behave as the reference's dict does: the later assignment wins, at the
        earlier one's position; the channels of the loser are ``shadowed``.  ``keepbits``: 1 .. 23, or None / "off"."""
        if keepbits in (None, "off"):
            keepbits = None
        elif isinstance(keepbits, bool) or not isinstance(keepbits, (int, np.integer)) or \
                not 1 <= int(keepbits) <= MANTISSA_BITS:
            raise ValueError(f"EncodeSpec: keepbits must be 1 .. {MANTISSA_BITS}, None or 'off'; got {keepbits!r}")
        else:
            keepbits = int(keepbits)
        names = [str(f) for f in names]
        levels = list(pressure_levels)
        column = {f: i for i, f in enumerate(names)}
        if len(column) != len(names):
            raise ValueError("EncodeSpec: channel names must be unique")

        def col(feature):
            if feature not in column:
                raise ValueError(f"EncodeSpec: configured output '{feature}' is not among the chunk's channels")
            return column[feature]

        chosen: Dict[str, Tuple[bool, Tuple[int, ...]]] = {}       # insertion-ordered, as the reference's data_vars
        shadowed: List[str] = []
        for v in cfg.features.output.atmospheric:
            out = ATMOSPHERIC_RENAMES.get(v, v)
            src = tuple(col(f"{v}_h{_level_tag(l)}") for l in levels)
            if out in chosen:
                shadowed += [names[c] for c in chosen[out][1]]
            chosen[out] = (False, src)
        for v in cfg.features.output.surface:
            if v in SKIPPED_SURFACE:
                continue
            out = SURFACE_RENAMES.get(v, v)
            if out in chosen:
                shadowed += [names[c] for c in chosen[out][1]]
            chosen[out] = (True, (col(v),))
        if dewpoint:
            if not levels:
                raise ValueError("EncodeSpec: dewpoint_depression needs pressure levels")
            chosen[DEWPOINT_NAME] = (False, tuple(-1 - l for l in range(len(levels))))
        variables, first = [], 0
        for name, (surface, src) in chosen.items():
            variables.append(Variable(name, len(src), surface, src, first))
            first += len(src)
        table = np.zeros(first, dtype=ENCODE_PLANE_DTYPE)
        for v in variables:
            rows = table[v.first:v.first + v.levels]
            rows["src"], rows["first"], rows["levels"], rows["level"] = v.sources, v.first, v.levels, np.arange(v.levels)
        return cls(names, levels, keepbits, bool(dewpoint), variables, shadowed, table)

    # ------------------------------------------------------------------ layout
    def numel(self, B: int, n_td: int, H: int, W: int) -> int:
        """elements of the encoded buffer"""
        return int(B) * int(n_td) * self.n_planes * int(H) * int(W)

    def block(self, v: Variable, B: int, n_td: int, H: int, W: int) -> Tuple[int, int]:
        """(first element, elements) of a variable's block"""
        per = int(B) * int(n_td) * int(H) * int(W)
        return v.first * per, v.levels * per

    def views(self, buffer, B: int, n_td: int, H: int, W: int) -> dict:
        """name -> view of the variable's block, ``[B, n_td, L, H, W]`` (atmospheric) or ``[B, n_td, H, W]`` (surface):
        the ``data_vars`` of the reference.  ``buffer``: the encoded buffer, a tensor (device or host) or a numpy array."""
        flat = buffer.reshape(-1)
        if flat.shape[0] < self.numel(B, n_td, H, W):
            raise ValueError(f"EncodeSpec.views: the buffer has {flat.shape[0]} elements, "
                             f"{self.numel(B, n_td, H, W)} are needed")
        out = {}
        for v in self.variables:
            a, m = self.block(v, B, n_td, H, W)
            shape = (B, n_td, H, W) if v.surface else (B, n_td, v.levels, H, W)
            out[v.name] = flat[a:a + m].reshape(shape)
        return out

    def template(self, n_time: int, forecast_steps: int, output_frequency: int, H: int, W: int) -> dict:
        """The float variables of ``_build_template_dataset``: per variable its dims, full shape and chunking, plus
        ``total_pred_steps`` (the stored steps and the initial state) and ``keepbits``.  Host only."""
        stored = (int(forecast_steps) - 1) // int(output_frequency) + 1
        total = stored + 1
        td = min(CHUNK_TIMEDELTAS, total)
        variables = {}
        for v in self.variables:
            if v.surface:
                variables[v.name] = {"dims": SFC_DIMS, "shape": (n_time, total, H, W), "chunks": (1, td, H, W)}
            else:
                variables[v.name] = {"dims": ATM_DIMS, "shape": (n_time, total, v.levels, H, W),
                                     "chunks": (1, td, v.levels, H, W)}
        return {"variables": variables, "total_pred_steps": total, "keepbits": self.keepbits, "dtype": "float32"}

    def device_table(self, device) -> torch.Tensor:
        return (self._dev.get(device) or device_tables(self._dev, device, device, (self.table.view(np.uint8),)))[0]


def pred_slice(start_idx: int, n: int, with_init: bool = True) -> slice:
    """The ``prediction_timedelta`` slice of a chunk of ``n`` stored states from stored step ``start_idx``
    (``write_forecast_region_chunked``): slot 0 is the initial state, which the first chunk carries."""
    if start_idx == 0 and with_init:
        return slice(0, 1 + n)
    return slice(1 + start_idx, 1 + start_idx + n)


def regions(sample_indices, sample_index_to_sorted_pos, start_idx: int, n: int) -> List[Region]:
    """``write_forecast_region_chunked`` without the write: the samples of the batch in ascending order, split into runs
    of consecutive positions on the store's sorted time axis; per run the batch rows, the ``time`` slice and the
    ``prediction_timedelta`` slice.  ``sample_index_to_sorted_pos``: the map of ``_get_sorted_time_info``.  Host only."""
    idx = np.asarray(sample_indices).reshape(-1)
    order = np.argsort(idx)
    pos = np.asarray(sample_index_to_sorted_pos)[idx[order]]
    breaks = np.where(np.diff(pos) != 1)[0] + 1
    td = pred_slice(int(start_idx), int(n))
    out = []
    for g in np.split(np.arange(len(pos)), breaks):
        if len(g):
            out.append(Region(order[g], slice(int(pos[g[0]]), int(pos[g[-1]]) + 1), td))
    return out


def encode_chunk(chunk: torch.Tensor, dew: Optional[torch.Tensor], spec: EncodeSpec, out: torch.Tensor, n_td: int,
                 td_off: int) -> None:
    """Time slots ``[td_off, td_off + n)`` of every variable's block ``[B, n_td, L_v, H, W]`` in ``out`` = the chunk's
    channels (and the dew-point levels) regrouped and BitRounded, by one launch of ``paradis_forecast_encode`` on the
    current stream; no host synchronisation, the sources are not written.

    chunk [B, n, C, H, W] fp32 with dense states (any batch / time stride); dew [B, n, L, H, W] or None; out: a
    contiguous float32 device tensor of at least ``spec.numel(B, n_td, H, W)`` elements (``spec.views`` names its
    blocks).  Algorithmic HBM bytes: 8 * B * n * spec.n_planes * H * W."""
    require_hip(chunk, dew, out)
    if chunk.dim() != 5:
        raise ValueError("encode_chunk: chunk [B, n, C, H, W] expected")
    B, n, C, H, W = chunk.shape
    L = spec.num_levels
    if C != spec.num_channels:
        raise ValueError(f"encode_chunk: a chunk of {C} channels for a spec of {spec.num_channels}")
    dense_state(chunk, "chunk", "encode_chunk", fp32=True)
    if spec.dewpoint:
        if dew is None:
            raise ValueError("encode_chunk: the spec writes dewpoint_depression and needs the dew-point chunk")
        if tuple(dew.shape) != (B, n, L, H, W):
            raise ValueError(f"encode_chunk: dew must be {(B, n, L, H, W)}, got {tuple(dew.shape)}")
        dense_state(dew, "dew", "encode_chunk", fp32=True)
    else:
        dew = None
    if not out.is_contiguous():
        raise ValueError("encode_chunk: out must be contiguous")
    if not (0 <= td_off and td_off + n <= n_td):
        raise ValueError(f"encode_chunk: slots [{td_off}, {td_off + n}) outside the {n_td} slots of a block")
    if out.numel() < spec.numel(B, n_td, H, W):
        raise ValueError(f"encode_chunk: out has {out.numel()} elements, {spec.numel(B, n_td, H, W)} are needed")
    P = H * W

    def strides(t, state):          # (batch, time): the time axis has its dense value too when it has one entry
        ts = t.stride(1) if n > 1 else state
        return batch_stride(t, n * ts), ts

    cbs, cts = strides(chunk, C * P)
    dbs, dts = strides(dew, L * P) if dew is not None else (0, 0)
    _lib.call("forecast_encode", 8.0 * B * n * spec.n_planes * P, dptr(chunk), cbs, cts, dptr(dew), dbs, dts,
              dptr(spec.device_table(chunk.device)), spec.table.ctypes.data, spec.n_planes, dptr(out), out.numel(),
              B, n, C, L, H, W, int(n_td), int(td_off), spec.keepbits_code, stream_ptr())


def initial_state(dataset, indices, post_spec, lat_deg, lon_deg):
    """The state the reference's writer puts in front of the first chunk (``init_data`` of
    ``_build_dataset_for_samples``): ``(state [B, 1, C, H, W], dew [B, 1, L, H, W])`` on the device, raw physical units
    of the store at the samples' init times - store row ``base + n_time_inputs - 1 + idx * interval_steps`` - in the
    chunk's channel order.  Output features that are not among the single-time input features are NaN.  Winds are
    converted and the dew point derived exactly as ``forecast.postprocess`` does them, with every normalisation kind 0.

    dataset: a ``dataset.DeviceDataset``; post_spec: the forecaster's ``PostSpec`` (its names are the dataset's output
    features).  Runs once per run: composed from the batch-assembly launch (a gather without normalisation) and the
    post-processing launch, no kernel of its own."""
    from .dataset import PLANE_DTYPE, assemble_planes
    from .forecast import postprocess
    if list(post_spec.names) != list(dataset.dyn_output_features):
        raise ValueError("initial_state: the PostSpec's names are not the dataset's output features")
    store = dataset.store
    T, F, H, W = store.shape
    C, L = post_spec.num_channels, post_spec.num_levels
    inputs = set(dataset.dyn_input_features)
    column = {name: j for j, name in enumerate(store.features)}
    missing = [c for c, f in enumerate(post_spec.names) if f not in inputs]
    table = np.zeros(C, dtype=PLANE_DTYPE)          # kind 0: the stored value; a missing plane reads column 0, then NaN
    table["feature"] = [0 if f not in inputs else column[f] for f in post_spec.names]
    table["dt"] = dataset.n_time_inputs - 1
    idx = dataset._indices(indices)
    B = int(idx.numel())
    dev = store.device
    with torch.inference_mode(False), torch.no_grad():
        planes = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        raw = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        state = torch.empty(B, 1, C, H, W, dtype=torch.float32, device=dev)
        dew = torch.empty(B, 1, L, H, W, dtype=torch.float32, device=dev) if post_spec.dewpoint else None
        if B == 0:
            return state, dew
        assemble_planes(store, idx, dataset.base, dataset.interval_steps, planes, 1, C, 0, 0, raw, None, dataset._flag)
        if missing:
            raw[:, missing] = float("nan")
        spec0 = dataclasses.replace(post_spec, kind=np.full_like(post_spec.kind, KIND_NONE))
        postprocess(raw, spec0, lat_deg, lon_deg, state, 0, dew)
    return state, dew
