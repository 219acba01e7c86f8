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

from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, _tables
from ._lib import dptr, require_hip, stream_ptr
from ._tables import batch_stride, dense_state, trig_tables
from .feed import KIND_HUMIDITY, KIND_ZSCORE, base_name, kind_of
from .rollout import ChunkRing, Stepper

UNIT_SINGLE, UNIT_LEVEL, UNIT_SURFACE = 0, 1, 2
_UNIT_INTS = 8


def var_indices(variable_name: str, variable_list: Sequence[str]) -> List[int]:
    """Positions of ``variable_name`` in a feature list with the ``_h<level>`` suffix stripped
    (reference utils/postprocessing.py:125-131)."""
    return [i for i, var in enumerate(variable_list) if base_name(var) == variable_name]


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
    _dev: dict = field(default_factory=dict, init=False, repr=False)      # (init=False: a replace() starts empty)
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
            kind[i] = kind_of(f, custom_normalization)
            if kind[i] == KIND_HUMIDITY:
                if q_min is None or q_max is None:
                    raise ValueError("custom_normalization with specific_humidity channels needs q_min and q_max")
                p0[i], p1[i] = float(q_min), float(q_max)
            elif kind[i] == KIND_ZSCORE:
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
        return self._dev.get(device) or _tables.device_tables(self._dev, device, device, (
            self.kind, self.p0, self.p1, self.units.reshape(-1), np.asarray(self.pressure_levels or [0.0], np.float64)))

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
    work = 8.0 * B * C * P + (4.0 * B * L * P if dew is not None else 0.0)
    _lib.call("forecast_post", work, dptr(output), batch_stride(output, C * P), dptr(chunk),
              batch_stride(chunk, T * C * P), slot * chunk.stride(1), dptr(dew),
              batch_stride(dew, T * L * P) if dew is not None else 0,
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
def _passed(scorecard, spectra, events, fractions, ensemble=None, probability=None, seeps=None) -> list:
    """the verification tables given to ``run`` (``_leadtable.LeadTable``: each brings its phrases, its ``members`` and
    whether its ``update`` takes ``clim_index``), in the order of their refusals and of their launches"""
    return [t for t in (scorecard, spectra, events, fractions, ensemble, probability, seeps) if t is not None]


def table_inputs(table, state, truth, clim_col) -> tuple:
    """what ``table.update`` gets behind the lead for one stored state: the finished ``state`` ``[B, C, H, W]``, the truth
    ``[B, C, H, W]`` of every ``table.members``-th batch entry - each ensemble's FIRST member: the members of one ensemble
    share their truth and their valid time - and, where the table takes one and the run has one, the same entries of the
    ``clim_index`` column ``[B]``.  Views only; pure."""
    m = table.members                                    # (1: ``x[::1]`` is ``x``'s address, shape and strides)
    clim = (clim_col[::m],) if table.TAKES_CLIM_INDEX and clim_col is not None else ()
    return (state, truth[::m]) + clim


class Forecaster:
    """``LitParadis.predict_step`` (reference trainer.py:731-815) on the device.

    ``run(input_data [B,1,n_inputs*num_common,H,W], forcings [B,S,H,W,F], constants [B,1,H,W,K], on_chunk)`` rolls the
    model out for S steps under ``torch.no_grad()`` (``rollout.Stepper``; ``graph=True``: a step is one forcing copy and
    one HIP-graph replay that honours parameters written in place between runs); every ``output_frequency``-th output
    goes through ``postprocess`` into the current chunk on the device; a finished chunk is copied by a side stream into
    pinned host memory (``rollout.ChunkRing``) and ``on_chunk(forecast=<numpy [B,n,C,H,W]>, start_idx=<int>,
    dewpoint=<numpy [B,n,L,H,W] or None>)`` is called - the arguments of the reference's ``write_forecast_chunk``.  The
    arrays are views of the pinned tensors, valid until ``on_chunk`` returns.  A chunk is handed over when the next one
    has been enqueued (or at the end), so the rollout does not wait for the copy or for the writer.  ``on_chunk=None``:
    the chunks are computed and copied but not handed over, and ``run`` returns without waiting for the device.

    ``run(..., scorecard=<verify.Scorecard>, truth=<[B, n_stored, C, H, W] on the device>, truth_normalized=False,
    clim_index=<int32 [B, n_stored] or None>)``: right after the post-processing of stored state ``k`` the finished state
    is scored in place against ``truth[:, k]`` at lead ``k`` (``scorecard.update``, one launch pair on the main stream, in
    front of the event the side-stream copy waits for).  ``truth_normalized=True``: the truth is in model space (a
    validation batch's ``true_data``) and goes through the same ``postprocess`` into a scratch state first.  A scorecard
    without ``truth``, or a truth of another ``n_stored``, is refused before the rollout starts.

    Six more tables go beside or without a scorecard, each under its own keyword, any subset of the seven in one run.
    The rule is one (``table_inputs``): the same finished state and the same truth state (one ``postprocess`` of a
    model-space truth serves all) go through each ``table.update`` at lead ``k``, with the ``clim_index`` column where
    the table takes one, on the main stream in the order below, in front of the same event.  An ensemble table
    (``members`` > 1) scores the batch of ``B = G * members`` states as ``G`` ensembles, member-minor (member ``i`` of
    ensemble ``g`` is batch entry ``g * members + i``): ``truth`` and ``clim_index`` keep their shapes, the table gets
    ``t[::members]`` and ``clim_index[::members, k]`` - the truth and the climatology slot of each ensemble's FIRST
    member; the members share their truth and valid time, the other members' entries are not read.  The refusals are
    the scorecard's for every table - no ``truth``, a truth of another shape, fewer leads than stored states, names
    that are not ``PostSpec.names`` (``all_names``; a ``channels=`` subset is the table's own business) - and, for an
    ensemble table, a ``B`` that is no multiple of its ``members``.
        ``spectra=<spectrum.Spectra>``                        one launch pair; takes no ``clim_index``
        ``events=<events.EventTable>``                        one launch pair
        ``fractions=<neighbourhood.FractionsTable>``          three launches
        ``ensemble=<ensemble.EnsembleCard>``                  one launch pair; ``members``; takes no ``clim_index``
        ``probability=<probability.ProbabilityTable>``        one launch pair; ``members``
        ``seeps=<seeps.SeepsTable>``                          three launches; ``clim_index``: the slots of its own
                                                              ``SeepsClimatology`` (one plan serves every table of a run)

    ``run(..., encoder=<encode.EncodeSpec>, init=<(state [B, 1, C, H, W], dew [B, 1, L, H, W] or None) or None>)``: a
    flushed chunk is regrouped into the writer's named variables and BitRounded on the device (``encode.encode_chunk``,
    one launch on the main stream) into a ring of its own, which is handed over in place of the plain chunk, with the
    same timing: ``on_chunk(variables=<dict name -> numpy view [B, n_td, (L,) H, W]>, start_idx=<int>,
    pred_slice=<slice>)``.  With ``init`` (``encode.initial_state``) the first chunk carries that state in slot 0
    (``n_td = n + 1``, ``pred_slice = slice(0, 1 + n)``, as the reference's writer); without it, and for every later
    chunk, ``n_td = n`` and ``pred_slice = slice(1 + start_idx, 1 + start_idx + n)``.  A scorecard keeps scoring the
    un-encoded state.  Refused before the rollout starts: an encoder whose names are not ``PostSpec.names``, one with
    ``dewpoint=True`` on a forecaster without the dew point, an ``init`` of another shape."""

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
        self._stepper = Stepper(model, self.num_common, self.n_inputs, self.graph)
        self._steps = self._stepper.steps      # (B, H, W) -> rollout.GraphedStep
        self._rings = {}       # (device, pair shapes) -> rollout.ChunkRing
        self._truth = {}       # (B, C, H, W, device) -> [B, 1, C, H, W]: a model-space truth state in physical units

    def _ring(self, device, shapes, pinned=True) -> ChunkRing:
        """the ring of these pairs, kept per shape; ``pinned=False``: no pinned tensors until a run hands this ring over"""
        key = (str(device), tuple(shapes.items()))
        ring = self._rings.get(key) or self._rings.setdefault(key, ChunkRing(device, shapes))
        ring.pending.clear()           # (a run that ended in an exception may have left some)
        return ring.pin() if pinned else ring

    def _check_verification(self, scorecard, truth, truth_normalized, clim_index, B, n_stored, C, H, W, spectra=None,
                            events=None, fractions=None, ensemble=None, probability=None, seeps=None):
        """the refusals of ``run(scorecard=..., spectra=..., events=..., fractions=..., ensemble=..., probability=...,
        seeps=...)``, before the rollout starts;
        returns the forecaster's ``[B, 1, C, H, W]`` scratch tensor for a model-space truth (``truth_normalized=True``),
        else None"""
        tables = _passed(scorecard, spectra, events, fractions, ensemble, probability, seeps)
        if not tables:
            if truth is not None or clim_index is not None or truth_normalized:
                raise ValueError("Forecaster.run: truth, truth_normalized and clim_index go with a scorecard")
            return None
        if clim_index is not None and not any(t.TAKES_CLIM_INDEX for t in tables):
            raise ValueError("Forecaster.run: clim_index goes with a scorecard")
        if truth.dim() != 5 or tuple(truth.shape) != (B, n_stored, C, H, W) or truth.dtype != torch.float32:
            raise ValueError(f"Forecaster.run: truth must be float32 {(B, n_stored, C, H, W)} (n_stored = {n_stored} "
                             f"stored states), got {truth.dtype} {tuple(truth.shape)}")
        for t in tables:
            if t.n_leads < n_stored:
                raise ValueError(f"Forecaster.run: {t.HAS} {t.n_leads} leads, the rollout stores {n_stored}")
            if list(t.all_names) != list(self.spec.names):
                raise ValueError(f"Forecaster.run: {t.NOUN}'s names are not the chunk's channel names (PostSpec.names)")
        for t in tables:
            if t.members > 1 and B % t.members != 0:
                raise ValueError(f"Forecaster.run: {t.HAS} {t.members} members, a batch of {B} states is not whole "
                                 f"ensembles")
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

    @torch.no_grad()
    def run(self, input_data, forcings, constants, on_chunk: Optional[Callable],
            forecast_steps: Optional[int] = None, *, scorecard=None, truth: Optional[torch.Tensor] = None,
            truth_normalized: bool = False, clim_index: Optional[torch.Tensor] = None, encoder=None, init=None,
            spectra=None, events=None, fractions=None, ensemble=None, probability=None, seeps=None):
        tables = _passed(scorecard, spectra, events, fractions, ensemble, probability, seeps)
        for t in tables:                                     # (host-side refusals, in front of the device checks)
            if truth is None:
                raise ValueError(f"Forecaster.run: {t.NEEDS} truth [B, n_stored, C, H, W] on the device")
        require_hip(input_data, forcings, constants)
        S = int(forcings.shape[1] if forecast_steps is None else forecast_steps)
        if forcings.shape[1] < S:
            raise ValueError(f"{S} forecast steps need as many forcing steps, got {forcings.shape[1]}")
        plan = chunk_plan(S, self.output_frequency, self.write_every_n)
        n_stored = sum(p.stored for p in plan)
        B, _, _, H, W = input_data.shape
        C, L = self.spec.num_channels, self.spec.num_levels
        truth_phys = self._check_verification(scorecard, truth, truth_normalized, clim_index, B, n_stored, C, H, W,
                                              spectra, events, fractions, ensemble, probability, seeps)
        init = self._check_encoder(encoder, init, B, C, L, H, W)
        sizes = [p.flush[1] for p in plan if p.flush is not None]         # per chunk its number of states
        n_chunk, sizes = max(sizes), iter(sizes)
        shapes = {"state": (B, n_chunk, C, H, W), **({"dew": (B, n_chunk, L, H, W)} if self.dewpoint else {})}
        ring = chunks = self._ring(input_data.device, shapes, pinned=encoder is None)   # (written, handed over)
        if encoder is not None:
            from .encode import encode_chunk, pred_slice
            # (axis 1 is not time: numel is linear in n_td, so a chunk's blocks [B, n_td, L_v, H, W] are a dense prefix)
            ring = self._ring(input_data.device, {"encoded": (1, n_chunk + 1, encoder.numel(B, 1, H, W))})

        def hand_over(start, n, host):             # (rollout.ChunkRing: rule 4)
            if encoder is None:
                on_chunk(forecast=host["state"].numpy(), start_idx=start,
                         dewpoint=host["dew"].numpy() if self.dewpoint else None)
            else:
                e = host["encoded"]
                on_chunk(variables=encoder.views(e.numpy(), B, e.shape[1], H, W), start_idx=start,
                         pred_slice=pred_slice(start, n, with_init=init is not None))

        self._stepper.begin(input_data, forcings, constants)
        i_stored = 0
        for step, p in enumerate(plan):
            out = self._stepper.step(step)
            if p.stored:
                if p.slot == 0:
                    views = chunks.open(next(sizes))
                    d, dd = views["state"], views.get("dew")
                postprocess(out, self.spec, self.lat_deg, self.lon_deg, d, p.slot, dd)
                if tables:
                    t = truth[:, i_stored]
                    if truth_phys is not None:             # a model-space truth: to physical units first
                        postprocess(t, self.spec, self.lat_deg, self.lon_deg, truth_phys, 0)
                        t = truth_phys[:, 0]
                    k = None if clim_index is None else clim_index[:, i_stored]
                    for table in tables:         # (scorecard, .., ensemble, probability, seeps: the launch order)
                        table.update(i_stored, *table_inputs(table, d[:, p.slot], t, k))
                i_stored += 1
            if p.flush is not None:
                start, n = p.flush
                if encoder is not None:
                    n_td, td_off = (n + 1, 1) if (start == 0 and init is not None) else (n, 0)   # the init state's slot
                    enc = ring.open(n_td)["encoded"]
                    if td_off:
                        encode_chunk(init[0], init[1], encoder, enc, n_td, 0)
                    encode_chunk(d, dd if encoder.dewpoint else None, encoder, enc, n_td, td_off)
                ring.flush(p.flush)
                ring.deliver(on_chunk and hand_over)       # chunk i-1: chunk i+1 will be copied into its pinned tensors
        ring.deliver(on_chunk and hand_over, keep=0)
        self._stepper.end()
