"""The forecast path: the reference's second entry point, ``forecast.py`` ->
``LitParadis.predict_step`` (reference ``trainer.py:731-815``), restated without Lightning - a no-grad autoregressive
rollout, every ``output_frequency``-th state kept, chunks of ``write_every_n`` stored states de-normalised
(``utils/postprocessing.py:190-215``), their Cartesian winds turned back into ``u, v, w``
(``utils/postprocessing.py:74-122,143-187``) and handed to a writer, plus the dew-point depression the reference's
writer derives (``utils/mhuaes.py`` through ``utils/file_output.py:165-173``).

The reference post-processes on the CPU after a ``.cpu()`` of the normalised chunk.  Here one HIP kernel
(``csrc/post.hip``) reads each stored model output once and writes the finished physical-unit state into its slot of
the chunk on the device; the chunk reaches the host finished.  With ``graph=True`` the forward step (input assembly,
model, feedback copy) is one HIP-graph replay.

No CPU fallback: the tensors must live on the HIP device.  fp32 only (the reference's ``forecast.py:85`` forces
``use_amp = False``).
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, harness
from ._lib import dptr, require_hip, stream_ptr
from ._tables import dense_state, trig_tables
from .feed import KIND_HUMIDITY, KIND_PRECIP, KIND_ZSCORE

UNIT_SINGLE, UNIT_LEVEL, UNIT_SURFACE = 0, 1, 2
_UNIT_INTS = 8


def var_indices(variable_name: str, variable_list: Sequence[str]) -> List[int]:
    """Positions of ``variable_name`` in a feature list with the ``_h<level>`` suffix stripped
    (reference utils/postprocessing.py:125-131)."""
    return [i for i, var in enumerate(variable_list) if re.sub(r"_h\d+$", "", var) == variable_name]


@dataclass
class PostSpec:
    """Host tables of ``paradis_forecast_post`` for one output feature list (device copies are made once per device)."""
    names: List[str]
    pressure_levels: List[float]
    kind: np.ndarray            # [C] int32, codes of feed.normalize_features_
    p0: np.ndarray              # [C] float32: mean | q_min
    p1: np.ndarray              # [C] float32: std  | q_max
    eps_q: float
    it: List[int]               # per level: channel of temperature, wind_x, wind_y, wind_z, specific humidity
    ix: List[int]
    iy: List[int]
    iz: List[int]
    iq: List[int]
    sfc: List[int]              # [wind_x_10m, wind_y_10m, wind_z_10m] or []
    winds: bool
    dewpoint: bool
    units: np.ndarray           # [U, 8] int32
    _dev: dict = field(default_factory=dict, repr=False)
    _trig: dict = field(default_factory=dict, repr=False)

    @property
    def num_channels(self) -> int:
        return len(self.names)

    @property
    def num_levels(self) -> int:
        return len(self.pressure_levels)

    @classmethod
    def from_features(cls, output_names: Optional[Sequence[str]], pressure_levels: Sequence[float], *, zscore_mean,
                      zscore_std, q_min=None, q_max=None, custom_normalization: bool = True, eps_q: float = 1e-12,
                      winds: bool = True, dewpoint: bool = True) -> "PostSpec":
        """Tables from the output feature names, found exactly as the reference finds them: normalisation classes as
        ``data/era5_dataset.py:463-523`` (``zscore_mean`` / ``zscore_std`` are indexed by position among the z-score
        channels, as ``output_mean[norm_zscore_out]`` is; with ``custom_normalization=False`` every channel is
        z-scored), wind / temperature / humidity channels as ``utils/postprocessing.py:150-158``, paired with
        ``pressure_levels`` by position.  ``output_names=None``: ``config.feature_layout(default_config())``'s order."""
        if output_names is None:
            from .config import default_config, feature_layout
            output_names = feature_layout(default_config()).output_name_order
        names = list(output_names)
        levels = [float(v) for v in pressure_levels]
        C, L = len(names), len(levels)
        kind = np.zeros(C, np.int32)
        p0 = np.zeros(C, np.float32)
        p1 = np.ones(C, np.float32)
        zs = []
        for i, f in enumerate(names):
            base = re.sub(r"_h\d+$", "", f)
            if base == "total_precipitation_6hr" and custom_normalization:
                kind[i] = KIND_PRECIP
            elif base == "specific_humidity" and custom_normalization:
                if q_min is None or q_max is None:
                    raise ValueError("custom_normalization with specific_humidity channels needs q_min and q_max")
                kind[i], p0[i], p1[i] = KIND_HUMIDITY, float(q_min), float(q_max)
            else:
                kind[i] = KIND_ZSCORE
                zs.append(i)
        mean = np.asarray(torch.as_tensor(zscore_mean).detach().cpu().numpy(), np.float32).reshape(-1)
        std = np.asarray(torch.as_tensor(zscore_std).detach().cpu().numpy(), np.float32).reshape(-1)
        if mean.size != len(zs) or std.size != len(zs):
            raise ValueError(f"zscore_mean / zscore_std need one entry per z-score channel ({len(zs)}); "
                             f"got {mean.size} / {std.size}")
        p0[zs], p1[zs] = mean, std
        it, iq = var_indices("temperature", names), var_indices("specific_humidity", names)
        ix, iy, iz = (var_indices(v, names) for v in ("wind_x", "wind_y", "wind_z"))
        sfc = [var_indices(v, names) for v in ("wind_x_10m", "wind_y_10m", "wind_z_10m")]
        if winds:
            for nm, idx in (("wind_x", ix), ("wind_y", iy), ("wind_z", iz), ("temperature", it)):
                if len(idx) != L:
                    raise ValueError(f"{len(idx)} {nm} channels for {L} pressure levels")
            if any(len(s) > 1 for s in sfc) or len({len(s) for s in sfc}) != 1:
                raise ValueError("wind_x_10m / wind_y_10m / wind_z_10m must appear once each or not at all")
        if dewpoint:
            for nm, idx in (("specific_humidity", iq), ("temperature", it)):
                if len(idx) != L:
                    raise ValueError(f"{len(idx)} {nm} channels for {L} pressure levels")
        sfc = [s[0] for s in sfc] if (winds and sfc[0]) else []
        units, used = [], set()
        if winds or dewpoint:
            for l in range(L):
                q = iq[l] if dewpoint else -1
                x, y, z = (ix[l], iy[l], iz[l]) if winds else (-1, -1, -1)
                units.append([UNIT_LEVEL, q, it[l], x, y, z, l, 0])
                used.update(c for c in (q, it[l], x, y, z) if c >= 0)
        if sfc:
            units.append([UNIT_SURFACE, -1, -1, sfc[0], sfc[1], sfc[2], 0, 0])
            used.update(sfc)
        if sum(1 for u in units for c in u[1:6] if c >= 0) != len(used):
            raise ValueError("a channel belongs to more than one level / wind group")
        units += [[UNIT_SINGLE, c, -1, -1, -1, -1, 0, 0] for c in range(C) if c not in used]
        return cls(names, levels, kind, p0, p1, float(eps_q), it, ix, iy, iz, iq, sfc, bool(winds), bool(dewpoint),
                   np.asarray(units, np.int32).reshape(-1, _UNIT_INTS))

    def device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            with torch.inference_mode(False):
                self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (
                    self.kind, self.p0, self.p1, self.units.reshape(-1),
                    np.asarray(self.pressure_levels or [0.0], np.float64)))
        return self._dev[key]

    def trig_tables(self, lat_deg, lon_deg, device):
        """the double sin / cos tables of the grid on ``device``, built once (``_tables.trig_tables``)"""
        return trig_tables(self._trig, lat_deg, lon_deg, device)


def postprocess(output: torch.Tensor, spec: PostSpec, lat_deg, lon_deg, chunk: torch.Tensor, slot: int,
                dew: Optional[torch.Tensor] = None) -> None:
    """``chunk[:, slot] = physical units of output`` (and ``dew[:, slot]`` = dew-point depression per level) by one launch
    of ``paradis_forecast_post`` on the current stream; no host synchronisation, ``output`` is not written.

    output [B, C, H, W] normalised fp32 (any batch stride); chunk [B, T, C, H, W]; dew [B, T, L, H, W] or None;
    lat_deg [H], lon_deg [W] in degrees.  Algorithmic HBM bytes: 8*B*C*H*W (+ 4*B*L*H*W with ``dew``)."""
    require_hip(output, chunk, dew)
    if output.dim() != 4 or chunk.dim() != 5:
        raise ValueError("postprocess: output [B, C, H, W] and chunk [B, T, C, H, W] expected")
    B, C, H, W = output.shape
    T = chunk.shape[1]
    if C != spec.num_channels or tuple(chunk.shape) != (B, T, C, H, W) or not 0 <= slot < T:
        raise ValueError(f"postprocess: output {tuple(output.shape)}, chunk {tuple(chunk.shape)}, slot {slot} and a "
                         f"{spec.num_channels}-channel spec do not fit together")
    dense_state(output, "output", "postprocess", fp32=True)
    dense_state(chunk, "chunk", "postprocess", fp32=True)
    P = H * W
    L = spec.num_levels
    if dew is not None:
        if not spec.dewpoint:
            raise ValueError("postprocess: dew-point output asked from a spec built with dewpoint=False")
        if tuple(dew.shape) != (B, T, L, H, W):
            raise ValueError(f"postprocess: dew must be {(B, T, L, H, W)}, got {tuple(dew.shape)}")
        dense_state(dew, "dew", "postprocess", fp32=True)
    trig, th, tw = spec.trig_tables(lat_deg, lon_deg, output.device)
    if (th, tw) != (H, W):
        raise ValueError(f"postprocess: lat/lon of {th} x {tw} points for a {H} x {W} state")
    kind, p0, p1, units, plev = spec.device_tables(output.device)

    def bs(t, state):
        return t.stride(0) if t.shape[0] > 1 else state

    work = 8.0 * B * C * P + (4.0 * B * L * P if dew is not None else 0.0)
    _lib.call("forecast_post", work, dptr(output), bs(output, C * P), dptr(chunk), bs(chunk, T * C * P),
              slot * chunk.stride(1), dptr(dew), bs(dew, T * L * P) if dew is not None else 0,
              slot * dew.stride(1) if dew is not None else 0, dptr(kind), dptr(p0), dptr(p1), spec.eps_q,
              dptr(units), spec.units.shape[0], dptr(plev), L, dptr(trig), B, C, H, W, stream_ptr())


# ---------------------------------------------------------------------------------- chunk bookkeeping
class StepPlan(NamedTuple):
    stored: bool                 # step % output_frequency == 0
    slot: int                    # position in the current chunk (-1 if not stored)
    flush: Optional[tuple]       # (start_idx, n_states) of the chunk handed over after this step, or None


def chunk_plan(forecast_steps: int, output_frequency: int, write_every_n: Optional[int] = None) -> List[StepPlan]:
    """The bookkeeping of ``predict_step`` (reference trainer.py:748-813) as a pure function: per step whether it is
    stored, its slot in the chunk, and the chunk flushed after it.  ``write_every_n`` defaults to ``forecast_steps``;
    ``start_idx`` counts stored steps; a trailing partial chunk is flushed after the last step."""
    S, freq = int(forecast_steps), int(output_frequency)
    n = S if write_every_n is None else int(write_every_n)
    if S < 1 or freq < 1 or n < 1:
        raise ValueError("chunk_plan: forecast_steps, output_frequency and write_every_n must be >= 1")
    plan, filled, start, stored_idx = [], 0, None, 0
    for step in range(S):
        stored, slot, flush = step % freq == 0, -1, None
        if stored:
            if start is None:
                start = stored_idx
            slot = filled
            filled += 1
            stored_idx += 1
            if filled == n:
                flush, filled, start = (start, n), 0, None
        if step == S - 1 and filled:
            flush, filled, start = (start, filled), 0, None
        plan.append(StepPlan(stored, slot, flush))
    return plan


# ---------------------------------------------------------------------------------- the predict loop
class _GraphedStep:
    """input assembly + model + feedback copy into the static input, captured once per (B, H, W)"""

    def __init__(self, model, inp, forc, const, num_common, n_inputs):
        with torch.inference_mode(False), torch.no_grad():
            self.inp, self.forc, self.const = (torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)
                                               for t in (inp, forc, const))      # dense, whatever the views' strides

            def step():
                mi = harness.assemble_model_input(self.inp.unsqueeze(1), self.forc.unsqueeze(1), self.const.unsqueeze(1))
                y = model(mi)
                self.inp.copy_(harness.next_input(mi, y, num_common, n_inputs))
                return y
            self.graph, self.out = harness.capture_forward(step)

    def load(self, inp, const):
        self.inp.copy_(inp, non_blocking=True)
        self.const.copy_(const, non_blocking=True)

    def __call__(self, forc_step):
        self.forc.copy_(forc_step, non_blocking=True)
        self.graph.replay()
        return self.out


class Forecaster:
    """``LitParadis.predict_step`` (reference trainer.py:731-815) on the device.

    ``run(input_data [B,1,n_inputs*num_common,H,W], forcings [B,S,H,W,F], constants [B,1,H,W,K], on_chunk)`` rolls the
    model out for S steps under ``torch.no_grad()``; every ``output_frequency``-th output goes through ``postprocess``
    into the current chunk on the device; a finished chunk is copied by a side stream into one of two pinned host
    buffers and ``on_chunk(forecast=<numpy [B,n,C,H,W]>, start_idx=<int>, dewpoint=<numpy [B,n,L,H,W] or None>)`` is
    called - the arguments of the reference's ``write_forecast_chunk``.  The arrays are views of the pinned buffers,
    valid until ``on_chunk`` returns.  A chunk is handed over when the next one has been enqueued (or at the end), so
    the rollout does not wait for the copy or for the writer.  ``on_chunk=None``: the chunks are computed and copied but
    not handed over, and ``run`` returns without waiting for the device (warm-up, timing).

    ``graph=True``: the forward step is captured into a HIP graph per (B, H, W) after an eager warm-up, outside
    ``ops.frozen_weights()`` - the weight-image kernels are nodes of the graph, so parameters written in place between
    runs (``load_state_dict``, an optimiser step) are honoured by the next replay.  Per step the host then issues one
    forcing copy, one replay and (stored steps) one post-processing launch.

    ``run(..., scorecard=<verify.Scorecard>, truth=<[B, n_stored, C, H, W] on the device>, truth_normalized=False,
    clim_index=<int32 [B, n_stored] or None>)``: right after the post-processing of stored state ``k`` the finished state
    is scored in place against ``truth[:, k]`` at lead ``k`` (``scorecard.update``, one launch pair on the main stream, in
    front of the event the side-stream copy waits for).  ``truth_normalized=True``: the truth is in model space (a
    validation batch's ``true_data``) and goes through the same ``postprocess`` into a scratch state first.  Without a
    scorecard ``run`` issues exactly the launches it issued before; a scorecard without ``truth``, or a truth of another
    ``n_stored``, is refused before the rollout starts.

    ``run(..., encoder=<encode.EncodeSpec>, init=<(state [B, 1, C, H, W], dew [B, 1, L, H, W] or None) or None>)``: a
    flushed chunk is regrouped into the writer's named variables and BitRounded on the device (``encode.encode_chunk``,
    one launch on the main stream in front of the event the side-stream copy waits for) into one of two encoded device
    buffers; the side stream copies that buffer - not the plain chunk - into one of two pinned buffers of the same layout
    and ``on_chunk(variables=<dict name -> numpy view [B, n_td, (L,) H, W]>, start_idx=<int>, pred_slice=<slice>)`` is
    called with the hand-over timing described above.  With ``init`` (``encode.initial_state``) the first chunk carries
    that state in slot 0 (``n_td = n + 1``, ``pred_slice = slice(0, 1 + n)``, as the reference's writer); without it,
    and for every later chunk, ``n_td = n`` and ``pred_slice = slice(1 + start_idx, 1 + start_idx + n)``.  A scorecard
    keeps scoring the un-encoded state.  Refused before the rollout starts: an encoder whose names are not
    ``PostSpec.names``, one with ``dewpoint=True`` on a forecaster without the dew point, an ``init`` of another shape.
    Without ``encoder`` ``run`` issues exactly the launches it issued before."""

    def __init__(self, model, spec: PostSpec, lat_deg, lon_deg, *, num_common: int = 83, n_inputs: int = 2,
                 output_frequency: int = 1, write_every_n: Optional[int] = None, graph: bool = True,
                 dewpoint: Optional[bool] = None):
        self.model, self.spec = model, spec
        self.lat_deg = np.asarray(lat_deg.detach().cpu() if isinstance(lat_deg, torch.Tensor) else lat_deg)
        self.lon_deg = np.asarray(lon_deg.detach().cpu() if isinstance(lon_deg, torch.Tensor) else lon_deg)
        self.num_common, self.n_inputs = int(num_common), int(n_inputs)
        self.output_frequency, self.write_every_n = int(output_frequency), write_every_n
        self.graph = bool(graph)
        self.dewpoint = spec.dewpoint if dewpoint is None else bool(dewpoint)
        self._steps = {}       # (B, H, W) -> _GraphedStep
        self._bufs = {}        # chunk shape -> device chunks, pinned buffers, events
        self._truth = {}       # (B, C, H, W, device) -> [B, 1, C, H, W]: a model-space truth state in physical units
        self._enc = {}         # chunk shape -> two encoded device buffers, two pinned buffers of the same layout

    def _buffers(self, B, n, C, L, H, W, device, pinned=True):
        """device chunks, pinned buffers, events; ``pinned=False`` (the encoded hand-over, which has pinned buffers of its
        own layout) leaves the plain pinned buffers unallocated until a run needs them"""
        key = (B, n, C, L, H, W, str(device), self.dewpoint)
        with torch.inference_mode(False):
            if key not in self._bufs:
                dev = [torch.empty(B, n, C, H, W, device=device) for _ in range(2)]
                ddev = [None, None]
                if self.dewpoint:
                    ddev = [torch.empty(B, n, L, H, W, device=device) for _ in range(2)]
                self._bufs[key] = (dev, [None, None], ddev, [None, None], [torch.cuda.Event() for _ in range(2)],
                                   [torch.cuda.Event() for _ in range(2)], torch.cuda.Stream(device=device),
                                   [False, False])
            host, dhost = self._bufs[key][1], self._bufs[key][3]
            if pinned and host[0] is None:
                host[:] = [torch.empty(B, n, C, H, W, pin_memory=True) for _ in range(2)]
                if self.dewpoint:
                    dhost[:] = [torch.empty(B, n, L, H, W, pin_memory=True) for _ in range(2)]
        return self._bufs[key]

    def _check_verification(self, scorecard, truth, truth_normalized, clim_index, B, n_stored, C, H, W):
        """the refusals of ``run(scorecard=...)``, before the rollout starts; returns the forecaster's ``[B, 1, C, H, W]``
        scratch tensor for a model-space truth (``truth_normalized=True``), else None"""
        if scorecard is None:
            if truth is not None or clim_index is not None or truth_normalized:
                raise ValueError("Forecaster.run: truth, truth_normalized and clim_index go with a scorecard")
            return None
        if truth.dim() != 5 or tuple(truth.shape) != (B, n_stored, C, H, W) or truth.dtype != torch.float32:
            raise ValueError(f"Forecaster.run: truth must be float32 {(B, n_stored, C, H, W)} (n_stored = {n_stored} "
                             f"stored states), got {truth.dtype} {tuple(truth.shape)}")
        if scorecard.n_leads < n_stored:
            raise ValueError(f"Forecaster.run: the scorecard has {scorecard.n_leads} leads, the rollout stores {n_stored}")
        if list(scorecard.names) != list(self.spec.names):
            raise ValueError("Forecaster.run: the scorecard's names are not the chunk's channel names (PostSpec.names)")
        if clim_index is not None and (clim_index.dtype != torch.int32 or tuple(clim_index.shape) != (B, n_stored)):
            raise ValueError(f"Forecaster.run: clim_index must be int32 {(B, n_stored)}, got {clim_index.dtype} "
                             f"{tuple(clim_index.shape)}")
        require_hip(truth)
        if not truth_normalized:
            return None
        key = (B, C, H, W, str(truth.device))
        if key not in self._truth:
            with torch.inference_mode(False):
                self._truth[key] = torch.empty(B, 1, C, H, W, device=truth.device)
        return self._truth[key]

    def _check_encoder(self, encoder, init, B, C, L, H, W):
        """the refusals of ``run(encoder=...)``, before the rollout starts; returns ``init`` as ``(state, dew or None)``"""
        if encoder is None:
            if init is not None:
                raise ValueError("Forecaster.run: init goes with an encoder")
            return None
        if list(encoder.names) != list(self.spec.names):
            raise ValueError("Forecaster.run: the encoder's names are not the chunk's channel names (PostSpec.names)")
        if encoder.dewpoint and not self.dewpoint:
            raise ValueError("Forecaster.run: the encoder writes dewpoint_depression, the forecaster has no dew point")
        if encoder.num_levels != L:
            raise ValueError(f"Forecaster.run: the encoder has {encoder.num_levels} levels, the chunk {L}")
        if init is None:
            return None
        state, dew = init
        if not encoder.dewpoint:
            dew = None
        elif dew is None:
            raise ValueError("Forecaster.run: the encoder writes dewpoint_depression, init has no dew point")
        require_hip(state, dew)
        if tuple(state.shape) != (B, 1, C, H, W) or (dew is not None and tuple(dew.shape) != (B, 1, L, H, W)):
            raise ValueError(f"Forecaster.run: init must be ({(B, 1, C, H, W)}, {(B, 1, L, H, W)} or None)")
        return state, dew

    def _encoded_buffers(self, B, n, H, W, numel, device):
        """per chunk shape, like ``_buffers``: its events order the accesses to these too"""
        key = (B, n, H, W, numel, str(device))
        if key not in self._enc:
            with torch.inference_mode(False):
                self._enc[key] = ([torch.empty(numel, device=device) for _ in range(2)],
                                  [torch.empty(numel, pin_memory=True) for _ in range(2)])
        return self._enc[key]

    @torch.no_grad()
    def run(self, input_data, forcings, constants, on_chunk: Optional[Callable],
            forecast_steps: Optional[int] = None, *, scorecard=None, truth: Optional[torch.Tensor] = None,
            truth_normalized: bool = False, clim_index: Optional[torch.Tensor] = None, encoder=None, init=None):
        if scorecard is not None and truth is None:          # (a host-side refusal, in front of the device checks)
            raise ValueError("Forecaster.run: a scorecard needs truth [B, n_stored, C, H, W] on the device")
        require_hip(input_data, forcings, constants)
        S = int(forcings.shape[1] if forecast_steps is None else forecast_steps)
        if forcings.shape[1] < S:
            raise ValueError(f"{S} forecast steps need as many forcing steps, got {forcings.shape[1]}")
        plan = chunk_plan(S, self.output_frequency, self.write_every_n)
        n_stored = sum(p.stored for p in plan)
        B, _, _, H, W = input_data.shape
        C, L = self.spec.num_channels, self.spec.num_levels
        truth_phys = self._check_verification(scorecard, truth, truth_normalized, clim_index, B, n_stored, C, H, W)
        init = self._check_encoder(encoder, init, B, C, L, H, W)
        n_chunk = min(n_stored, S if self.write_every_n is None else int(self.write_every_n))
        dev, host, ddev, dhost, filled, copied, side, used = self._buffers(B, n_chunk, C, L, H, W, input_data.device,
                                                                            pinned=encoder is None)
        if encoder is not None:
            from .encode import encode_chunk, pred_slice
            enc, henc = self._encoded_buffers(B, n_chunk, H, W, encoder.numel(B, n_chunk + 1, H, W), input_data.device)
        main = torch.cuda.current_stream()
        const = constants[:, :1].permute(0, 1, 4, 2, 3)
        forc = forcings.permute(0, 1, 4, 2, 3)
        step_fn = None
        if self.graph:
            key = (B, H, W)
            if key not in self._steps:
                from . import ops
                with ops.frozen_weights(False):
                    self._steps[key] = _GraphedStep(self.model, input_data[:, 0], forc[:, 0], const[:, 0],
                                                    self.num_common, self.n_inputs)
            step_fn = self._steps[key]
            step_fn.load(input_data[:, 0], const[:, 0])
        cur = input_data
        # per chunk its number of states, known in advance: a trailing partial chunk uses a dense [B, n, ...] view of the
        # same storage, so every device-to-host copy is one contiguous transfer
        sizes = [p.flush[1] for p in plan if p.flush is not None]

        def views(j, n):
            def v(t, ch):
                return None if t is None else t.view(-1)[:B * n * ch * H * W].view(B, n, ch, H, W)
            return v(dev[j], C), v(host[j], C), v(ddev[j], L), v(dhost[j], L)

        def slots(start, n):         # (n_td, td_off) of a chunk's encoded blocks: the first one carries the init state
            return (n + 1, 1) if (start == 0 and init is not None) else (n, 0)

        def deliver(p):
            if on_chunk is None:
                return
            j, start, n = p
            copied[j].synchronize()
            if encoder is not None:
                n_td, _ = slots(start, n)
                on_chunk(variables=encoder.views(henc[j].numpy(), B, n_td, H, W), start_idx=start,
                         pred_slice=pred_slice(start, n, with_init=init is not None))
                return
            _, h, _, dh = views(j, n)
            on_chunk(forecast=h.numpy(), start_idx=start, dewpoint=dh.numpy() if self.dewpoint else None)

        pending = None         # (buffer index, start_idx, n) enqueued for copy, not yet handed over
        i_chunk = 0
        i_stored = 0
        for step, p in enumerate(plan):
            if step_fn is not None:
                out = step_fn(forc[:, step])
            else:
                mi = harness.assemble_model_input(cur, forc[:, step].unsqueeze(1), const)
                out = self.model(mi)
                cur = harness.next_input(mi, out, self.num_common, self.n_inputs).unsqueeze(1)
            k = i_chunk & 1
            if p.stored:
                if p.slot == 0:
                    d, h, dd, dh = views(k, sizes[i_chunk])
                    if used[k]:
                        main.wait_event(copied[k])     # the side stream has finished reading this device chunk
                postprocess(out, self.spec, self.lat_deg, self.lon_deg, d, p.slot, dd)
                if scorecard is not None:      # on the main stream, in front of `filled`: the copy sees a finished chunk
                    t = truth[:, i_stored]
                    if truth_phys is not None:
                        postprocess(t, self.spec, self.lat_deg, self.lon_deg, truth_phys, 0)
                        t = truth_phys[:, 0]
                    scorecard.update(i_stored, d[:, p.slot], t, None if clim_index is None else clim_index[:, i_stored])
                i_stored += 1
            if p.flush is not None:
                start, n = p.flush
                if encoder is not None:        # on the main stream, in front of `filled`, into the buffer `copied[k]` guards
                    n_td, td_off = slots(start, n)
                    if td_off:
                        encode_chunk(init[0], init[1], encoder, enc[k], n_td, 0)
                    encode_chunk(d, dd if encoder.dewpoint else None, encoder, enc[k], n_td, td_off)
                    m = encoder.numel(B, n_td, H, W)
                filled[k].record(main)
                with torch.cuda.stream(side):
                    side.wait_event(filled[k])
                    if encoder is not None:
                        henc[k][:m].copy_(enc[k][:m], non_blocking=True)
                    else:
                        h.copy_(d, non_blocking=True)
                        if self.dewpoint:
                            dh.copy_(dd, non_blocking=True)
                    copied[k].record(side)
                used[k] = True
                if pending is not None:
                    deliver(pending)               # chunk i-1; its pinned buffer is the one chunk i+1 will be copied into
                pending = (k, start, n)
                i_chunk += 1
        if pending is not None:
            deliver(pending)
