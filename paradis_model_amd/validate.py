"""The validation path: the reference's third entry loop, ``LitParadis.validation_step``
(reference ``trainer.py:652-708``), restated without Lightning - a no-grad autoregressive rollout over the ``S`` target
steps, per step the validation loss (``val_loss_fn``), the per-channel losses (``utils/loss.py:105-127``) and the
latitude-weighted RMSE in physical units of the configured report features (``_get_report_rmse``,
``trainer.py:291-315``), averaged over the steps and then over the epoch.

The reference evaluates these with a dozen full-size ATen passes per step and reads every logged value on the host.
Here one HIP launch pair (``csrc/score.hip``) reads the model output and the target view once and leaves all numbers of
the step in one row on the device; rows are accumulated on the device and read once, in ``Validator.result``.  With
``graph=True`` the forward step (input assembly, model, feedback copy) is one HIP-graph replay (``rollout.Stepper``).

No CPU fallback: the tensors must live on the HIP device.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, _tables
from ._lib import dptr, require_hip, stream_ptr
from ._tables import batch_stride, dense_state, sum_over_ranks, workspace
from .feed import KIND_HUMIDITY, KIND_PRECIP, KIND_ZSCORE
from .rollout import Stepper

LOSS_KIND = {"mse": 0, "reversed_huber": 1, "amse": 2}       # 2 = none: the AMSE value comes from ops.amse_loss


@dataclass
class ReportSpec:
    """Host tables of the report features of ``paradis_val_score`` (device copies are made once per device)."""
    names: List[str]
    chan: np.ndarray            # [R] int32: channel of each report feature
    cls: np.ndarray             # [R] int32: codes of feed.normalize_features_
    p0: np.ndarray              # [R] float32: q_min (humidity)
    p1: np.ndarray              # [R] float32: std (z-score) | q_max (humidity)
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def num_reports(self) -> int:
        return len(self.names)

    @classmethod
    def from_features(cls, report_features: Sequence[str], feature_names: Optional[Sequence[str]] = None, *,
                      report_std, custom_normalization: bool, q_min=None, q_max=None) -> "ReportSpec":
        """Tables chosen as the reference chooses its branches (trainer.py:277-283,297-313): the channel is the position
        of the name in ``feature_names`` (default ``config.feature_layout(default_config()).output_name_order``; the
        reference indexes ``dyn_input_features``, whose leading common block has the same positions); with custom
        normalisation ``"specific_humidity" in name`` selects the humidity class, then ``"precipitation" in name`` the
        precipitation class (substring tests, in this order); everything else is z-score with ``report_std[r]``
        (indexed by position in the report list).  An empty list is allowed, a feature may appear twice."""
        if feature_names is None:
            from .config import default_config, feature_layout
            feature_names = feature_layout(default_config()).output_name_order
        feature_names = list(feature_names)
        names = [str(f) for f in report_features]
        R = len(names)
        std = np.asarray(torch.as_tensor(report_std).detach().cpu().numpy(), np.float32).reshape(-1)
        if std.size != R:
            raise ValueError(f"report_std needs one entry per report feature ({R}); got {std.size}")
        chan, kind = np.zeros(R, np.int32), np.zeros(R, np.int32)
        p0, p1 = np.zeros(R, np.float32), np.ones(R, np.float32)
        for r, f in enumerate(names):
            if f not in feature_names:
                raise ValueError(f"report feature '{f}' is not among the feature names")
            chan[r] = feature_names.index(f)
            # (substring tests: the reference's own rule for reports, trainer.py:277-283 - not feed.kind_of's base names)
            if custom_normalization and "specific_humidity" in f:
                if q_min is None or q_max is None:
                    raise ValueError("custom_normalization with a specific_humidity report needs q_min and q_max")
                kind[r], p0[r], p1[r] = KIND_HUMIDITY, float(q_min), float(q_max)
            elif custom_normalization and "precipitation" in f:
                kind[r] = KIND_PRECIP
            else:
                kind[r], p1[r] = KIND_ZSCORE, std[r]
        first = {}
        for r in range(R):        # the kernel forms one sum per channel: a channel listed twice has one set of constants
            k = first.setdefault(int(chan[r]), r)
            if (kind[k], p0[k], p1[k]) != (kind[r], p0[r], p1[r]):
                raise ValueError(f"report feature '{names[r]}' is listed twice with different statistics")
        return cls(names, chan, kind, p0, p1)

    def device_tables(self, device, C: int):
        """(rflag [C], rcls [C], rp0 [C], rp1 [C], rchan [R]) on ``device``"""
        key = (device, int(C))
        if key not in self._dev:
            if self.num_reports and int(self.chan.max()) >= C:
                raise ValueError(f"report channel {int(self.chan.max())} outside a {C}-channel state")
            rflag, rcls = np.full(C, -1, np.int32), np.zeros(C, np.int32)
            rp0, rp1 = np.zeros(C, np.float32), np.ones(C, np.float32)
            for r in range(self.num_reports - 1, -1, -1):
                c = int(self.chan[r])
                rflag[c], rcls[c], rp0[c], rp1[c] = r, self.cls[r], self.p0[r], self.p1[r]
            rchan = self.chan if self.num_reports else np.zeros(1, np.int32)
            _tables.device_tables(self._dev, key, device, (rflag, rcls, rp0, rp1, rchan))
        return self._dev[key]


_WS: Dict[tuple, torch.Tensor] = {}


def row_size(C: int, R: int) -> int:
    return 1 + 2 * C + R


def score(pred: torch.Tensor, target: torch.Tensor, loss, reports: Optional[ReportSpec],
          out_row: torch.Tensor) -> None:
    """``out_row[1 + 2C + R]`` = (loss, per-channel loss weighted [C], unweighted [C], report RMSE [R]) of one step, by one
    launch pair of ``paradis_val_score`` on the current stream; no host synchronisation, neither input is written.

    pred, target [B, C, H, W] normalised fp32, any batch stride (``true_data[:, step]`` and a channel slice of a wider
    tensor are consumed in place); ``loss`` a ``ParadisLoss`` on the device: ``out_row[0]`` is ``loss(pred, target)``,
    ``out_row[1:1+C]`` / ``[1+C:1+2C]`` are ``loss.per_channel_loss(pred, target, weighted=True / False)``; for an
    ``"amse"`` loss these 1 + 2C entries are zeros (the caller fills ``out_row[0]`` from ``loss(pred, target)``).
    Reports use ``loss.lat_weights`` whether or not the loss applies latitude weights, as the reference does.
    Algorithmic HBM bytes: 8*B*C*H*W."""
    require_hip(pred, target, out_row)
    if pred.dim() != 4 or target.shape != pred.shape:
        raise ValueError(f"score: pred and target must be [B, C, H, W] of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    B, C, H, W = pred.shape
    R = reports.num_reports if reports is not None else 0
    if out_row.dim() != 1 or out_row.numel() != row_size(C, R) or out_row.stride(0) != 1:
        raise ValueError(f"score: out_row must be a dense vector of 1 + 2*{C} + {R} entries")
    dense_state(pred, "pred", "score")
    dense_state(target, "target", "score")
    wf = loss.feature_weights_buf.reshape(-1)
    lat = loss.lat_weights_buf.reshape(-1)
    require_hip(wf, lat)
    if wf.numel() != C or lat.numel() != H:
        raise ValueError(f"score: the loss was built for {wf.numel()} channels and {lat.numel()} latitudes, got a "
                         f"{C} x {H} x {W} state")
    wl = lat if loss.apply_latitude_weights else None
    P = H * W
    tabs = reports.device_tables(pred.device, C) if R else (None,) * 5
    chan_h = reports.chan.ctypes.data_as(ctypes.c_void_p) if R else None
    cls_h = reports.cls.ctypes.data_as(ctypes.c_void_p) if R else None
    ws = workspace(_WS, pred.device, int(_lib.lib.paradis_val_score_ws_bytes(B, C, H, W)))
    _lib.call("val_score", 8.0 * B * C * P, dptr(pred), batch_stride(pred, C * P), dptr(target),
              batch_stride(target, C * P), dptr(wf), dptr(wl),
              dptr(lat) if R else None, LOSS_KIND[loss.kind], float(loss.delta), chan_h, cls_h, R,
              *(dptr(t) for t in tabs), dptr(out_row), dptr(ws), B, C, H, W, stream_ptr())


class Validator:
    """``LitParadis.validation_step`` (reference trainer.py:652-708) and the epoch means Lightning forms from it.

    ``step(batch)``, batch = ``(input_data [B,1,n_inputs*num_common,H,W], true_data [B,S,C,H,W], forcings [B,S,H,W,F],
    constants [B,1,H,W,K])``: rolls the model out over the S target steps under ``torch.no_grad()`` (also inside
    ``torch.inference_mode()``), scores every output against ``true_data[:, step]`` into row ``step`` of a device tensor
    ``[S, 1 + 2C + R]`` (``score``) and returns that tensor.  The batch value - the mean over the steps,
    trainer.py:686,701 - is added to device accumulators with weight B, Lightning's epoch mean.  Nothing in ``step``
    waits for the device.

    ``result(sync_dist=False)`` reads the accumulators once and returns ``{"val_loss", <report feature name>...,
    "val_loss_channel_weighted/<name>"..., "val_loss_channel_unweighted/<name>"...}``; with ``sync_dist=True`` and an
    initialised process group the accumulator vector and its weight are summed over the ranks by ONE all-reduce first
    (the reference: one per logged value).  ``reset()`` clears the accumulators.

    ``graph=True``: forward and feedback copy are one HIP-graph replay per step that honours an optimiser step between
    two validations (``rollout.Stepper``); scoring runs outside the graph.  ``amp=True``: the forward runs under
    ``torch.autocast(bfloat16)``; the output is scored in fp32.  An ``"amse"`` validation loss: row entry 0 is
    ``val_loss(out, target)`` (``ops.amse_loss``), the per-channel entries are zeros.  ``keep_outputs=True`` keeps
    clones of the last ``step``'s outputs in ``self.outputs``."""

    def __init__(self, model, val_loss, reports: Optional[ReportSpec] = None, *, num_common: int = 83,
                 n_inputs: int = 2, graph: bool = True, amp: bool = False, keep_outputs: bool = False):
        self.model, self.val_loss, self.reports = model, val_loss, reports
        self.num_common, self.n_inputs = int(num_common), int(n_inputs)
        self.graph, self.amp, self.keep_outputs = bool(graph), bool(amp), bool(keep_outputs)
        self.channel_names = list(val_loss.output_name_order)
        self.outputs: List[torch.Tensor] = []
        self._stepper = Stepper(self._forward, self.num_common, self.n_inputs, self.graph)
        self._steps = self._stepper.steps      # (B, H, W) -> rollout.GraphedStep
        self._acc = None       # float64 [1 + 2C + R] on the device: sum over batches of B * (mean over steps)
        self._weight = 0       # sum of B (host: the batch size is known without the device)

    def _forward(self, mi):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.amp):
            y = self.model(mi)
        return y if y.dtype == torch.float32 else y.float()

    @torch.no_grad()
    def step(self, batch) -> torch.Tensor:
        input_data, true_data, forcings, constant_data = batch
        require_hip(input_data, true_data, forcings, constant_data)
        B, S, C, H, W = true_data.shape
        if forcings.shape[1] < S:
            raise ValueError(f"{S} target steps need as many forcing steps, got {forcings.shape[1]}")
        R = self.reports.num_reports if self.reports is not None else 0
        n = row_size(C, R)
        with torch.inference_mode(False):
            rows = torch.empty(S, n, device=true_data.device)
            if self._acc is None or self._acc.numel() != n or self._acc.device != true_data.device:
                self._acc, self._weight = torch.zeros(n, dtype=torch.float64, device=true_data.device), 0
        self._stepper.begin(input_data, forcings, constant_data)
        amse = self.val_loss.kind == "amse"
        if self.keep_outputs:
            self.outputs = []
        for s in range(S):
            out = self._stepper.step(s)
            target = true_data[:, s]
            score(out, target, self.val_loss, self.reports, rows[s])
            if amse:
                rows[s, :1].copy_(self.val_loss(out, target).reshape(1))
            if self.keep_outputs:
                self.outputs.append(out.clone())
        self._stepper.end()
        self._acc.add_(rows.sum(dim=0, dtype=torch.float64), alpha=float(B) / S)
        self._weight += B
        return rows

    def reset(self) -> None:
        if self._acc is not None:
            self._acc.zero_()
        self._weight = 0

    def result(self, sync_dist: bool = False) -> Dict[str, float]:
        if self._acc is None or self._weight == 0:
            raise RuntimeError("Validator.result: no batch has been scored since the last reset")
        n = self._acc.numel()
        acc, weight = self._acc, float(self._weight)
        if sync_dist:          # the accumulators and their weight travel as one vector
            vec = sum_over_ranks(torch.cat([acc, acc.new_tensor([weight])]), True)
            acc, weight = vec[:n], float(vec[n])
        v = (acc.cpu() / weight).tolist()
        C = len(self.channel_names)
        res = {"val_loss": v[0]}
        if self.reports is not None:
            for r, name in enumerate(self.reports.names):
                res[name] = v[1 + 2 * C + r]
        for c, name in enumerate(self.channel_names):
            res[f"val_loss_channel_weighted/{name}"] = v[1 + c]
            res[f"val_loss_channel_unweighted/{name}"] = v[1 + C + c]
        return res
