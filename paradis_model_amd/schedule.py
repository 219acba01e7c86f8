"""Learning-rate schedules that a captured training step can follow (reference ``trainer.py:366-456``).

The reference steps its scheduler on the host after every optimiser step (``"interval": "step"``) and the optimiser reads
``group["lr"]``.  A HIP graph captured around the step (``harness.GraphedTrainStep``) cannot: a host scalar would be frozen
into the kernel arguments, and pushing a new value between replays (``optim.AdamW.sync_device_state``) is a blocking
host-to-device copy that drains the queue on every step of a warm-up or a decay.  A schedule that is a pure function of the
step number - the reference's warm-up / steady / decay ``LambdaLR`` - is instead tabulated once, uploaded once, and read on
the device: one launch per optimiser step (``paradis_lr_schedule``) writes every group's learning rate for ITS step count
into the group's device state, inside the graph.

OneCycleLR (which also cycles ``betas[0]``) and ReduceLROnPlateau (per epoch, driven by a validation metric) keep the
host route: set ``group["lr"]``, then ``optimizer.sync_device_state()``.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch


def wsd_lambda(total_steps, warmup, decay) -> Callable[[int], float]:
    """The multiplier of the reference's warm-up / steady / decay schedule (``trainer.py:416-449``) as a function of the
    0-based scheduler step.  ``warmup`` / ``decay``: a value >= 1 is a number of steps, a value < 1 a fraction of
    ``total_steps``.  Rising ``(step + 1) / warmup_steps`` below the warm-up, 1 up to and including step
    ``warmup_steps + steady_steps``, then ``(total_steps - step) / decay_steps``."""
    warmup_steps = warmup if warmup >= 1 else warmup * total_steps
    decay_steps = decay if decay >= 1 else decay * total_steps
    if not warmup_steps >= 0:
        raise AssertionError("wsd: warmup_steps >= 0")
    if not decay_steps >= 0:
        raise AssertionError("wsd: decay_steps >= 0")
    if not warmup_steps + decay_steps <= total_steps:
        raise AssertionError("wsd: warmup_steps + decay_steps <= total_steps")
    steady_steps = total_steps - (warmup_steps + decay_steps)

    def lr_lambda(step):
        if step < warmup_steps:
            return (step + 1) / warmup_steps
        if step <= warmup_steps + steady_steps:
            return 1.0
        return (total_steps - step) / decay_steps

    return lr_lambda


class Schedule:
    """a multiplier ``lr_lambda(k)`` of the base learning rate and the number of optimiser steps it is tabulated for"""

    def __init__(self, lr_lambda: Callable[[int], float], total_steps: int):
        self.lr_lambda, self.total_steps = lr_lambda, int(total_steps)


def from_config(scheduler_cfg, total_steps) -> Optional[Schedule]:
    """``cfg.training.scheduler`` -> the ``Schedule`` that runs on the device (``wsd.enabled``), or ``None``: OneCycleLR and
    ReduceLROnPlateau stay host-side schedulers (module docstring)."""
    def enabled(name):
        sub = scheduler_cfg.get(name, None) if hasattr(scheduler_cfg, "get") else getattr(scheduler_cfg, name, None)
        return bool(sub is not None and sub.get("enabled", False))
    if sum(enabled(n) for n in ("one_cycle", "reduce_lr", "wsd")) != 1:
        raise ValueError("Invalid config: Exactly one scheduler must be enabled")
    if not enabled("wsd"):
        return None
    wsd = scheduler_cfg.get("wsd")
    return Schedule(wsd_lambda(total_steps, wsd.get("warmup"), wsd.get("decay")), total_steps)


def as_schedule(schedule) -> Schedule:
    """a ``Schedule`` or a ``(lr_lambda, total_steps)`` pair"""
    if isinstance(schedule, Schedule):
        return schedule
    lr_lambda, total_steps = schedule
    return Schedule(lr_lambda, total_steps)


class DeviceSchedule:
    """The learning rates of every parameter group of ``optimizer`` for optimiser steps ``1 .. total_steps``:
    ``table[g][k] = float32(base_lr_g * lr_lambda(k))`` - the product in Python double, rounded once - is what
    ``torch.optim.lr_scheduler.LambdaLR`` stepped once per optimiser step leaves in ``group["lr"]`` before optimiser
    step ``k + 1``, as the device holds it (fp32).  ``base_lr_g`` is ``group["lr"]`` at construction.  Past the end of the
    table its last entry holds.

    ``host_lr(g, k)``: that number as a Python float (the eager twin of a graphed run, logging).
    ``apply()``: the launch; an optimiser it is attached to (``optim.AdamW.attach_schedule``) calls it inside ``step()``
    behind the ticks of the groups' device step counts.  The table (4 bytes per step and group: 1.2 MB per group at
    300,000 steps) and the addresses of the groups' device states are uploaded at the first call, which therefore must
    not be inside a graph capture (``GraphedTrainStep`` runs eager warm-up steps first)."""

    def __init__(self, optimizer, lr_lambda: Callable[[int], float], total_steps: int):
        n = int(total_steps)
        if n < 1:
            raise ValueError("DeviceSchedule: total_steps must be at least 1")
        self.optimizer = optimizer
        self.total_steps = n
        self.base_lrs = [float(g["lr"]) for g in optimizer.param_groups]
        lam = [float(lr_lambda(k)) for k in range(n)]
        # [G][n]: the LambdaLR values in double, and what the device holds
        self.values64 = np.array([[base * m for m in lam] for base in self.base_lrs], dtype=np.float64).reshape(-1, n)
        self.table = self.values64.astype(np.float32)
        self._dev = None           # (key, device table, device address table)

    def host_lr(self, group_index: int, k: int) -> float:
        return float(self.table[group_index, min(max(int(k), 0), self.total_steps - 1)])

    def apply(self) -> None:
        from ._lib import check, dptr, lib, stream_ptr
        states = self.optimizer._dev_state
        G = len(self.base_lrs)
        addr = [states[gi][0].data_ptr() if gi in states else 0 for gi in range(G)]
        if not any(addr):
            return
        key = tuple(addr)
        if self._dev is None or self._dev[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceSchedule: the tables must be uploaded before a graph capture (run an eager step first)")
            dev = next(states[gi][0].device for gi in range(G) if gi in states)
            table = self._dev[1] if self._dev is not None else torch.from_numpy(self.table).to(dev)
            self._dev = (key, table, torch.tensor(addr, dtype=torch.int64, device=dev))
        _, table, addresses = self._dev
        check(lib.paradis_lr_schedule(dptr(addresses), dptr(table), G, self.total_steps, stream_ptr()), "lr_schedule")
