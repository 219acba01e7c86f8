"""Host side of the table-driven launches (``csrc/stream_common.h``): the chunk list of a tensor list, the address
table that reaches the device through a pinned staging row, the per-stream workspace cache and the dense-state check
of the plane kernels, and the trigonometric tables of the wind kernels.  The pinned-row protocol lives here once: ``optim.AdamW``, ``optim.Muon``, ``clip.ClipPlan`` and
``diagnostics.StatsPlan`` all go through ``AddressTable``."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist


def chunk_list(numels: Sequence[int], chunk: int, tensors=None) -> Tuple[List[int], List[int]]:
    """(chunk_tensor, chunk_off) as Python lists: one entry per ``chunk`` elements of every tensor, in tensor order
    (``tensors``: the indices to walk, default all), then by offset"""
    ct: List[int] = []
    co: List[int] = []
    for t in (range(len(numels)) if tensors is None else tensors):
        for off in range(0, int(numels[t]), chunk):
            ct.append(t)
            co.append(off)
    return ct, co


class AddressTable:
    """``rows`` rows of ``T`` int64 device addresses: ``host`` the pinned staging row, ``ptrs`` the device row the kernels
    read (row r of tensor t at ``ptrs[r * T + t]``), ``pending`` the event of the last asynchronous copy out of ``host``.

    The addresses change behind the same parameter ids (``zero_grad(set_to_none=True)``, ``load_state_dict``,
    ``model.to()``), so ``write`` rewrites all of them before every launch; nothing waits for the device."""

    def __init__(self, rows: int, T: int, device):
        n = max(1, rows * T)
        with torch.inference_mode(False):
            self.host = torch.zeros(n, dtype=torch.int64).pin_memory()
            self.ptrs = torch.zeros(n, dtype=torch.int64, device=device)
        self.n = rows * T
        self.pending = None

    def write(self, addresses: Sequence[int]) -> bool:
        """stage ``addresses`` (all rows, concatenated) and queue their copy to the device on the current stream; returns
        whether the stream is capturing (the copy is then a graph node that re-reads ``host`` on every replay)"""
        capturing = torch.cuda.is_current_stream_capturing()
        if self.pending is not None and not capturing:       # the previous call's async copy out of `host` (long done)
            self.pending.synchronize()
        if self.n:
            self.host.copy_(torch.tensor(addresses, dtype=torch.int64))
            self.ptrs.copy_(self.host, non_blocking=True)
            if capturing:
                self.pending = None      # (inside a capture the copy is a graph node; nothing to wait for on the host)
            else:
                ev = torch.cuda.Event()
                ev.record()
                self.pending = ev
        return capturing

    # ------------------------------------------------------------------ HIP graphs (harness.GraphedTrainStep.eager_step)
    def snapshot(self) -> torch.Tensor:
        """a copy of the pinned row (a captured copy node re-reads the row on every replay)"""
        return self.host.clone()

    def restore(self, table) -> None:
        if table is None or self.host.numel() != table.numel():
            return
        if self.pending is not None:
            self.pending.synchronize()
        self.host.copy_(table)


def workspace(cache: Dict[tuple, torch.Tensor], device, nbytes: int) -> torch.Tensor:
    """at least ``nbytes`` of device memory out of the owner's ``cache``, one buffer per (device, current stream): the
    launches of one stream are ordered, so they may share it; it grows when a call needs more"""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        with torch.inference_mode(False):
            ws = cache[key] = torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.float64, device=device)
    return ws


def dense_state(t: torch.Tensor, what: str, who: str, fp32: bool = False) -> None:
    """``t[..., C, H, W]`` holds dense ``[C, H, W]`` states (any stride in front of them); ``fp32``: and is float32.
    ``who`` / ``what`` name the caller and the argument in the error."""
    dense = t.stride(-1) == 1 and t.stride(-2) == t.shape[-1] and t.stride(-3) == t.shape[-1] * t.shape[-2]
    if fp32:
        if t.dtype != torch.float32 or not dense:
            raise ValueError(f"{who}: {what} must be float32 with dense [C, H, W] states")
    elif not dense:
        raise ValueError(f"{who}: {what} must hold dense [C, H, W] states")


def batch_stride(t: torch.Tensor, dense: int) -> int:
    """``t.stride(0)``, or ``dense`` when the batch axis has one entry (the stride of such an axis is arbitrary)"""
    return t.stride(0) if t.shape[0] > 1 else dense


def device_tables(cache: dict, key, device, arrays) -> tuple:
    """``cache[key]`` = the numpy ``arrays`` as a tuple of tensors on ``device``, made outside inference mode so that every
    later mode may read them.  For a miss: a launch-bound owner looks first (``cache.get(key) or device_tables(...)``)."""
    with torch.inference_mode(False):
        cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays)
    return cache[key]


def sum_over_ranks(t: torch.Tensor, sync_dist: bool) -> torch.Tensor:
    """``t`` on the host: with ``sync_dist`` and an initialised process group summed over the ranks by ONE all-reduce
    first (under gloo after the one device-to-host read, in front of the host-side sum).  ``t`` is not written."""
    if sync_dist and dist.is_available() and dist.is_initialized():
        t = (t.cpu() if dist.get_backend() == "gloo" else t).clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu()


def trig_tables(cache: dict, lat_deg, lon_deg, device):
    """(double [sin(lat)[H], cos(lat)[H], sin(lon)[W], cos(lon)[W]] on ``device``, H, W) out of the owner's ``cache``:
    built once per grid on the host with numpy from the 1-D degree arrays (float32 arrays are widened first: float64
    trigonometry of the stored values).  The tables of ``csrc/post.hip`` and ``csrc/prepare.hip``."""
    if isinstance(lat_deg, torch.Tensor):
        lat_deg = lat_deg.detach().cpu().numpy()
    if isinstance(lon_deg, torch.Tensor):
        lon_deg = lon_deg.detach().cpu().numpy()
    lat = np.ascontiguousarray(np.asarray(lat_deg, np.float64).reshape(-1))
    lon = np.ascontiguousarray(np.asarray(lon_deg, np.float64).reshape(-1))
    key = (str(device), lat.tobytes(), lon.tobytes())
    if key not in cache:
        la, lo = np.deg2rad(lat), np.deg2rad(lon)
        tab = np.concatenate([np.sin(la), np.cos(la), np.sin(lo), np.cos(lo)])
        with torch.inference_mode(False):
            cache[key] = (torch.from_numpy(tab).to(device), lat.size, lon.size)
    return cache[key]
