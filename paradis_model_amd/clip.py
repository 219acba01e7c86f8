"""Global-norm gradient clipping: the reference's ``training.gradient_clip_val`` (``train.py:52-53``, algorithm
``"norm"``), i.e. ``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False)``.

Under the reference's manual optimisation Lightning refuses the Trainer flag, so its users call ``clip_grad_norm_``
themselves between the last backward and ``opt.step()``: ``clip.clip_grad_norm_`` is that line.  On the HIP device it is
three launches (``csrc/clip.hip``: chunk partials in double, one finishing workgroup, one scale pass) where ATen's foreach
path runs 18 device activities over the default model's 335 gradients (measured); nothing waits for the device.  CPU parameters go through
``torch.nn.utils.clip_grad_norm_`` (the host logic of ``harness.TrainStep`` is tested that way, as the optimiser falls
back to ``torch.optim.AdamW`` there).
"""
from __future__ import annotations

import math
from typing import Iterable, Optional, Sequence, Union

import torch


def check_max_norm(max_norm) -> float:
    value = float(max_norm)
    if not math.isfinite(value) or value <= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be finite and > 0, got {max_norm!r}")
    return value


class ClipPlan:
    """Device tables of ``paradis_clip_grad_norm`` for one list of tensor sizes (they depend on nothing else), the pinned
    staging buffer of the gradient address row, the workspace and the result ``out`` = fp32 ``[2]`` on the device:
    ``{norm before clipping, coefficient}``."""

    def __init__(self, numels: Sequence[int], device):
        from . import _lib
        from ._tables import AddressTable, chunk_list
        self.T = len(numels)
        ct, co = chunk_list(numels, _lib.lib.paradis_clip_grad_chunk())
        self.n_chunks = len(ct)
        self.numel_host = [int(n) for n in numels]
        self.n_elements = sum(self.numel_host)
        self.addr = AddressTable(1, self.T, device)
        with torch.inference_mode(False):
            self.numel = torch.tensor([int(n) for n in numels] or [0], dtype=torch.int64, device=device)
            self.chunk_tensor = torch.tensor(ct or [0], dtype=torch.int32, device=device)
            self.chunk_off = torch.tensor(co or [0], dtype=torch.int64, device=device)
            ws = int(_lib.lib.paradis_clip_grad_ws_bytes(self.n_chunks))
            self.ws = torch.empty(max(1, ws // 8), dtype=torch.float64, device=device)
            self.out = torch.zeros(2, device=device)
        _lib.require_hip(self.out)

    def launch(self, grads, max_norm: float) -> torch.Tensor:
        """rewrite the address row (pinned staging buffer, non-blocking copy: the addresses change after
        ``zero_grad(set_to_none=True)``) and run the launches on the current stream; ``grads``: one entry per tensor of
        the plan, ``None`` = absent"""
        from . import _lib
        from ._lib import dptr, stream_ptr
        T = self.T
        grads = list(grads)
        if len(grads) != T:
            raise ValueError(f"clip_grad_norm_: the plan was built for {T} tensors, got {len(grads)}")
        max_norm = check_max_norm(max_norm)
        numel = self.numel_host
        addr = [0] * T
        for t, g in enumerate(grads):
            if g is None:
                continue
            if g.is_sparse or g.layout != torch.strided:
                raise RuntimeError("clip_grad_norm_: sparse gradients are not supported")
            if not g.is_cuda or g.device != self.out.device:
                raise RuntimeError(f"clip_grad_norm_: a gradient on {g.device}, the plan on {self.out.device}")
            if g.dtype != torch.float32:
                raise RuntimeError(f"clip_grad_norm_: gradients must be fp32, got {g.dtype}")
            if not g.is_contiguous():
                raise RuntimeError("clip_grad_norm_: non-contiguous gradient")
            if g.numel() != numel[t]:
                raise ValueError(f"clip_grad_norm_: a gradient of {g.numel()} elements where the plan has {numel[t]}")
            addr[t] = g.data_ptr()
        self.addr.write(addr)
        _lib.call("clip_grad_norm", 12.0 * self.n_elements, dptr(self.addr.ptrs), dptr(self.numel),
                  dptr(self.chunk_tensor), dptr(self.chunk_off), T, self.n_chunks, max_norm, dptr(self.ws),
                  dptr(self.out), stream_ptr())
        return self.out

    # ------------------------------------------------------------------ the pinned address row and HIP graphs
    def snapshot_pointer_tables(self):
        """a copy of the pinned address row (``harness.GraphedTrainStep``: the captured copy node re-reads it on every
        replay)"""
        return self.addr.snapshot()

    def restore_pointer_tables(self, table) -> None:
        self.addr.restore(table)


_PLANS: dict = {}          # parameter-list key -> ClipPlan, most recently used last
_MAX_PLANS = 8


def plan_for(params: Sequence[torch.Tensor]) -> ClipPlan:
    """the cached ``ClipPlan`` of this parameter list (keyed like ``optim.AdamW._fused_cache``: identities, sizes, device)"""
    dev = params[0].device
    key = tuple((id(p), p.numel()) for p in params) + (str(dev),)
    plan = _PLANS.pop(key, None)
    if plan is None:
        plan = ClipPlan([p.numel() for p in params], dev)
        while len(_PLANS) >= _MAX_PLANS:
            _PLANS.pop(next(iter(_PLANS)))
    _PLANS[key] = plan
    return plan


@torch.no_grad()
def clip_grad_norm_(parameters: Union[torch.Tensor, Iterable[torch.Tensor]], max_norm: float,
                    plan: Optional[ClipPlan] = None) -> torch.Tensor:
    """Scale the gradients of ``parameters`` in place so that their global 2-norm is at most ``max_norm``; returns fp32
    ``[2]`` = ``{norm before clipping, coefficient applied}`` on the parameters' device (with a plan: the plan's ``out``,
    overwritten by the next call).  Nothing waits for the device.

    Parameters without a gradient are skipped; a non-contiguous or non-fp32 gradient raises.  ``plan``: a ``ClipPlan``
    built for exactly these parameters' sizes, else the one cached for this parameter list.  CPU parameters go through
    ``torch.nn.utils.clip_grad_norm_``."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    max_norm = check_max_norm(max_norm)
    if not params:
        return torch.tensor([0.0, 1.0])
    if not any(p.is_cuda for p in params):
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False)
        norm = norm.to(torch.float32)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        return torch.stack([norm, coef])
    if not all(p.is_cuda for p in params):
        raise RuntimeError("clip_grad_norm_: parameters on the host and on the device in one call")
    if plan is None:
        plan = plan_for(params)
    return plan.launch([p.grad for p in params], max_norm)
