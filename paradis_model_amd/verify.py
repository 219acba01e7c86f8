"""Forecast verification: how RMSE, bias, MAE, anomaly correlation (ACC) and activity grow with lead time, for every
variable of a forecast chunk, in physical units - the deterministic scores of WeatherBench-2, accumulated on the device.

Conventions.  Forecast ``f`` and truth ``t`` are ``[B, C, H, W]`` fp32 in physical units, in the chunk layout of
``forecast.postprocess`` (with ``winds=True``: ``u, v, w`` where ``wind_x, wind_y, wind_z`` were).  ``w[h] >= 0`` are
latitude weights (``[H]``, not all zero), ``Z = W * sum_h w[h]`` (formed in double on the host).  An optional
climatology ``clim [K, C, H, W]`` comes with an index ``k[b]`` (int32 on the device, ``0 <= k < K``) that names the
climatology slot of sample ``b`` at this lead (``climatology.build`` makes both from a ``DeviceStore``).  Per sample ``b`` and channel ``c``, sums over the plane, with
``fa = f - clim[k[b]]`` and ``ta = t - clim[k[b]]``::

    se = sum w (f-t)^2 / Z      e  = sum w (f-t) / Z      ae = sum w |f-t| / Z
    ff = sum w fa^2             tt = sum w ta^2            ft = sum w fa ta
    acc_b = ft / sqrt(ff * tt)       (the sample is left out of the ACC mean when ff * tt == 0)

Accumulated per (lead, channel), eight doubles: ``{n, sum se, sum e, sum ae, sum acc_b, n_acc, sum ff, sum tt}``.
Reported: ``rmse = sqrt(sum se / n)``, ``bias = sum e / n``, ``mae = sum ae / n``, ``acc = sum acc_b / n_acc``,
``activity = sqrt(sum ff / sum tt)`` (the ratio of forecast to truth anomaly amplitude; it falls below 1 as a forecast
blurs) and ``count = n``.  Without a climatology ``acc`` and ``activity`` are NaN and no third tensor is read.
Non-finite values in ``f`` or ``t`` are NOT masked: they propagate into the scores of their (lead, channel).

One launch pair per ``update`` (``csrc/verify.hip``) reads the two (three) tensors once - 8 (12) bytes per cell - and
adds to one row of numbers kept on the device; ``result`` reads them once, after at most one all-reduce.

No CPU fallback: ``update`` needs tensors on the HIP device.  The host side (argument checks, ``result``, ``table``)
works on any device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr
from ._leadtable import LeadTable
from ._tables import batch_stride, sum_over_ranks, workspace

ACC_FIELDS = 8          # {n, sum se, sum e, sum ae, sum acc_b, n_acc, sum ff, sum tt}
METRICS = ("rmse", "bias", "mae", "acc", "activity")


def lat_weights_from(loss) -> torch.Tensor:
    """the latitude weights of a ``ParadisLoss`` (``loss.lat_weights_buf``), as ``Scorecard`` takes them"""
    return loss.lat_weights_buf


class Scorecard(LeadTable):
    """Per-lead verification scores of a rollout, accumulated on the device (module docstring for the formulas).

    ``names``: the chunk's channel names (``PostSpec.names``); ``lat_weights``: ``[H]`` (any shape with H entries);
    ``climatology``: ``[K, C, H, W]`` fp32 on the device, or ``None``.  ``acc`` is the double ``[n_leads, C, 8]``
    accumulator on ``device``.

    ``update(lead, forecast, truth, clim_index=None)``: one launch pair on the current stream, no host synchronisation,
    neither input is written; ``forecast`` / ``truth`` ``[B, C, H, W]`` fp32 with dense ``[C, H, W]`` states and any
    batch stride (``chunk[:, slot]`` and ``truth[:, k]`` are consumed in place); ``clim_index`` ``[B]`` int32 on the
    device (with a one-slot climatology it may be omitted).
    ``result(sync_dist=False)``: one device read; ``{"rmse", "bias", "mae", "acc", "activity"``: numpy float64
    ``[n_leads, C]``, ``"count"``: numpy ``[n_leads]``, ``"names"``: list``}``; leads never updated come back as NaN
    with count 0.  With ``sync_dist=True`` and an initialised process group ``acc`` is summed over the ranks by ONE
    all-reduce first (through the host under gloo, as ``Validator.result``).
    ``reset()`` clears the accumulators.  ``table(result, channels=None)``: a plain-text scorecard for logs."""

    IT = NOUN = "the scorecard"
    IT_HAS = HAS = "the scorecard has"
    NEEDS = "a scorecard needs"

    def __init__(self, names: Sequence[str], lat_weights, n_leads: int, *, climatology: Optional[torch.Tensor] = None,
                 device="cuda"):
        super().__init__(names, n_leads, device)
        w = torch.as_tensor(lat_weights).detach().reshape(-1)
        if w.numel() < 1 or not w.is_floating_point():
            raise ValueError("Scorecard: lat_weights must be a floating-point vector [H]")
        w64 = w.double().cpu()
        if not bool(torch.isfinite(w64).all()) or bool((w64 < 0).any()) or float(w64.sum()) <= 0.0:
            raise ValueError("Scorecard: lat_weights must be finite, >= 0 and not all zero")
        self._wsum = float(w64.sum())                       # Z = W * sum_h w[h], in double on the host
        self.H = w.numel()
        with torch.inference_mode(False):
            self.lat_w = w.to(device=self.device, dtype=torch.float32).contiguous().clone()
            self.acc = torch.zeros(self.n_leads, self.C, ACC_FIELDS, dtype=torch.float64, device=self.device)
        self._set_climatology(climatology, home=self.lat_w.device, same_index=True)

    lat_weights_from = staticmethod(lat_weights_from)

    def update(self, lead: int, forecast: torch.Tensor, truth: torch.Tensor,
               clim_index: Optional[torch.Tensor] = None) -> None:
        B, C, H, W = self._check(lead, forecast, truth, clim_index)
        require_hip(forecast, truth, self.lat_w)
        if B == 0:             # (empty tensors have no address to hand over; the entry point would do nothing either)
            return
        clim = self.climatology
        clim_index, K = self._clim_args(clim_index, forecast)
        P = H * W
        with_clim = clim is not None
        ws = workspace(self._ws, forecast.device, int(_lib.lib.paradis_verify_ws_bytes(B, C, H, W, int(with_clim))))
        _lib.call("verify_update", (12.0 if with_clim else 8.0) * B * C * P, dptr(forecast),
                  batch_stride(forecast, C * P), dptr(truth), batch_stride(truth, C * P), dptr(clim),
                  dptr(clim_index), K, dptr(self.lat_w), float(W) * self._wsum, dptr(self.acc[int(lead)]), dptr(ws),
                  B, C, H, W, stream_ptr())

    def reset(self) -> None:
        self.acc.zero_()

    def result(self, sync_dist: bool = False) -> dict:
        a = sum_over_ranks(self.acc, sync_dist).numpy()
        n, n_acc = a[..., 0], a[..., 5]
        with np.errstate(divide="ignore", invalid="ignore"):
            res = {"rmse": np.sqrt(a[..., 1] / n), "bias": a[..., 2] / n, "mae": a[..., 3] / n}
            if self.climatology is None:
                res["acc"] = np.full(n.shape, np.nan)
                res["activity"] = np.full(n.shape, np.nan)
            else:
                res["acc"] = a[..., 4] / n_acc
                res["activity"] = np.sqrt(a[..., 6] / a[..., 7])
        for k in METRICS:
            res[k] = np.where(n > 0, res[k], np.nan)        # leads never updated
        res["count"] = n[:, 0].copy()
        res["names"] = list(self.names)
        return res

    @staticmethod
    def table(result: dict, channels: Optional[Sequence[str]] = None) -> str:
        """plain text, one block per metric: a row per lead, a column per channel (``channels``: a subset, by name)"""
        names: List[str] = list(result["names"])
        chosen = names if channels is None else [str(c) for c in channels]
        for c in chosen:
            if c not in names:
                raise ValueError(f"Scorecard.table: channel '{c}' is not among the scorecard's names")
        cols = [names.index(c) for c in chosen]
        width = max([12] + [len(c) + 1 for c in chosen])
        lines = []
        for metric in METRICS:
            lines.append(f"{metric:<6}{'count':>8}" + "".join(f"{c:>{width}}" for c in chosen))
            for lead in range(result[metric].shape[0]):
                vals = "".join(f"{result[metric][lead, c]:>{width}.4e}" for c in cols)
                lines.append(f"{lead:<6d}{int(result['count'][lead]):>8d}" + vals)
            lines.append("")
        return "\n".join(lines[:-1])
