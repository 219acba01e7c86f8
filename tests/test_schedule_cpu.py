"""CPU: the learning-rate schedule tables (paradis_model_amd/schedule.py), the argument validation of the two C-ABI entries
behind a captured Muon / NorMuon step, and the host bookkeeping of a capturable Muon optimiser.

The warm-up / steady / decay multiplier is checked against the reference's rule (trainer.py:416-449, restated in
``_reference_lambda``) driven the way the reference drives it: ``torch.optim.lr_scheduler.LambdaLR`` stepped once per
optimiser step on a ``torch.optim.SGD``."""
import struct

import numpy as np
import pytest
import torch

from paradis_model_amd import schedule as S
from paradis_model_amd.config import to_attr


def _reference_lambda(total_steps, warmup, decay):
    warmup_steps = warmup if warmup >= 1 else warmup * total_steps
    decay_steps = decay if decay >= 1 else decay * total_steps
    assert warmup_steps >= 0
    assert decay_steps >= 0
    assert warmup_steps + decay_steps <= total_steps
    steady_steps = total_steps - (warmup_steps + decay_steps)

    def lr_lambda(step):
        if step < warmup_steps:
            return (step + 1) / warmup_steps
        elif step <= warmup_steps + steady_steps:
            return 1.0
        return (total_steps - step) / decay_steps
    return lr_lambda


def _lambda_lr_sequence(base_lrs, lr_lambda, total):
    """``group["lr"]`` of every group before optimiser steps 1 .. total under LambdaLR with interval "step" """
    groups = [dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=lr) for lr in base_lrs]
    opt = torch.optim.SGD(groups, lr=base_lrs[0])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda)
    seq = []
    for _ in range(total):
        seq.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sched.step()
    return np.array(seq, dtype=np.float64).T          # [G][total]


class _Groups:
    """the part of an optimiser that DeviceSchedule reads on the host"""

    def __init__(self, lrs):
        self.param_groups = [dict(lr=lr) for lr in lrs]


CASES = [(7, 3, 3), (8, 3, 0.25), (10, 0.2, 0.2),
         (6, 1, 2),          # warm-up of one step
         (8, 3, 5)]          # the decay spans everything after the warm-up


@pytest.mark.parametrize("total,warmup,decay", CASES)
def test_wsd_table_equals_lambda_lr(total, warmup, decay):
    base = 5e-4
    want = _lambda_lr_sequence([base], _reference_lambda(total, warmup, decay), total)
    ds = S.DeviceSchedule(_Groups([base]), S.wsd_lambda(total, warmup, decay), total)
    assert ds.values64.shape == (1, total) and ds.values64.dtype == np.float64
    assert np.array_equal(ds.values64, want), (ds.values64, want)
    assert ds.table.dtype == np.float32 and np.array_equal(ds.table, want.astype(np.float32))
    for k in range(total):
        assert ds.host_lr(0, k) == float(np.float32(want[0, k]))
    assert ds.host_lr(0, total + 5) == ds.host_lr(0, total - 1)       # past the end the last entry holds


def test_wsd_phases():
    lam = S.wsd_lambda(7, 3, 3)          # steady_steps = 1: 1.0 while step <= 4
    assert [lam(k) for k in range(7)] == [1 / 3, 2 / 3, 1.0, 1.0, 1.0, 2 / 3, 1 / 3]
    lam = S.wsd_lambda(8, 0, 0)
    assert [lam(k) for k in range(8)] == [1.0] * 8


def test_wsd_shipped_schedule_spot_checks():
    total, warmup, decay, base = 300000, 1000, 0.2, 5e-4
    ref = _reference_lambda(total, warmup, decay)
    ds = S.DeviceSchedule(_Groups([base]), S.wsd_lambda(total, warmup, decay), total)
    assert ds.table.shape == (1, total) and ds.table.nbytes == 4 * total
    for k in (0, 999, 1000, 239999, 240000, 240001, 299999):
        assert ds.values64[0, k] == base * ref(k), k
        assert ds.table[0, k] == np.float32(base * ref(k)), k
    assert ds.values64[0, 0] == base / 1000 and ds.values64[0, 999] == base and ds.values64[0, 240000] == base
    assert ds.values64[0, 240001] == base * (59999 / 60000.0) and ds.values64[0, 299999] == base * (1 / 60000.0)


@pytest.mark.parametrize("total,warmup,decay", [(10, 6, 5), (10, 0.6, 0.5), (10, -0.1, 2), (10, 2, -0.1)])
def test_wsd_invalid_combinations_raise(total, warmup, decay):
    with pytest.raises(AssertionError):
        _reference_lambda(total, warmup, decay)
    with pytest.raises(AssertionError):
        S.wsd_lambda(total, warmup, decay)


def test_two_groups_get_their_own_rows():
    total, lrs = 9, [2e-3, 5e-4]
    lam = S.wsd_lambda(total, 4, 3)
    want = _lambda_lr_sequence(lrs, _reference_lambda(total, 4, 3), total)
    ds = S.DeviceSchedule(_Groups(lrs), lam, total)
    assert ds.table.shape == (2, total)
    assert np.array_equal(ds.values64, want) and np.array_equal(ds.table, want.astype(np.float32))
    assert ds.host_lr(0, 4) == float(np.float32(2e-3)) and ds.host_lr(1, 4) == float(np.float32(5e-4))
    assert ds.host_lr(0, 0) != ds.host_lr(1, 0)


def test_from_config_selects_wsd():
    off = {"enabled": False}
    cfg = to_attr({"one_cycle": off, "reduce_lr": off, "wsd": {"enabled": True, "warmup": 1000, "decay": 0.2}})
    sch = S.from_config(cfg, 300000)
    ref = _reference_lambda(300000, 1000, 0.2)
    assert sch.total_steps == 300000
    assert all(sch.lr_lambda(k) == ref(k) for k in (0, 500, 1000, 240000, 240001, 299999))
    assert S.as_schedule(sch) is sch and S.as_schedule((ref, 7)).total_steps == 7
    # the host-side schedulers are not tabulated
    assert S.from_config(to_attr({"one_cycle": {"enabled": True}, "reduce_lr": off, "wsd": off}), 10) is None
    with pytest.raises(ValueError):
        S.from_config(to_attr({"one_cycle": {"enabled": True}, "reduce_lr": off, "wsd": {"enabled": True}}), 10)


def test_abi_validation_without_gpu():
    from paradis_model_amd import _lib
    L = _lib.lib
    tail = (0.1, 0.1, 0.95, 0.95, 0.0, 1e-8, 0, 0, 0, None, None, 1.0, None)
    assert L.paradis_muon_step_d(None, 2, 2, 0, 4, *tail) == 1                 # rows < 1
    assert "bad shape" in _lib.last_error()
    assert L.paradis_muon_step_d(None, 1, 2, 4, 4, *tail) == 1                 # stride < T
    assert L.paradis_muon_step_d(None, 2, 2, 4, 4, *tail) == 1                 # no table, no workspace
    assert "workspace" in _lib.last_error()
    assert L.paradis_muon_step_d(None, 2, 0, 4, 4, *tail) == 0                 # empty group
    assert L.paradis_lr_schedule(None, None, 2, 5, None) == 1
    assert "tables" in _lib.last_error()
    assert L.paradis_lr_schedule(None, None, -1, 5, None) == 1
    assert L.paradis_lr_schedule(None, None, 2, 0, None) == 1                  # an empty table has no last entry
    assert "bad arguments" in _lib.last_error()
    assert L.paradis_lr_schedule(None, None, 0, 5, None) == 0                  # no groups
    assert L.paradis_abi_version() == 10


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def test_capturable_muon_keys_device_state_by_group(monkeypatch):
    """[matrix, adamw] groups with different learning rates: the device state of each group is filed under its index
    in ``param_groups``, so ``sync_device_state()`` pushes each group's own rate (host bookkeeping only: the kernels
    are stubbed out, the "device" states are CPU tensors)."""
    from paradis_model_amd import optim
    w = torch.nn.Parameter(torch.zeros(4, 3))
    b = torch.nn.Parameter(torch.zeros(5))
    opt = optim.NorMuon([dict(params=[w], algorithm="normuon", lr=2e-3), dict(params=[b], algorithm="adamw", lr=5e-4)],
                        lr=1e-3, capturable=True)
    assert opt.capturable and isinstance(opt, optim.AdamW)
    assert not optim.Muon([torch.nn.Parameter(torch.zeros(2, 2))]).capturable
    w.grad, b.grad = torch.ones_like(w), torch.ones_like(b)
    ticked = []

    class _Lib:
        @staticmethod
        def paradis_adamw_tick(state, stream):
            ticked.append(state.value)
            return 0
    monkeypatch.setattr(optim, "lib", _Lib)
    monkeypatch.setattr(optim, "require_hip", lambda *a, **k: None)
    monkeypatch.setattr(optim, "stream_ptr", lambda: None)
    monkeypatch.setattr(optim.Muon, "_update_group", lambda self, pl: None)
    opt.step()
    assert set(opt._dev_state) == {0, 1}
    assert ticked == [opt._dev_state[0][0].data_ptr(), opt._dev_state[1][0].data_ptr()]
    assert opt._dev_state[0][0].tolist() == [0, _bits(2e-3)] and opt._dev_state[1][0].tolist() == [0, _bits(5e-4)]
    assert opt.state[w]["step"] == 1 and "momentum" in opt.state[w] and "exp_avg" in opt.state[b]
    # the host route: a scheduler changes the AdamW group's rate only
    opt.param_groups[1]["lr"] = 1e-4
    opt.sync_device_state()
    assert opt._dev_state[0][1] == 2e-3 and opt._dev_state[0][0][1].item() == _bits(2e-3)
    assert opt._dev_state[1][1] == 1e-4 and opt._dev_state[1][0][1].item() == _bits(1e-4)
    # a replay advances the step count of the momentum states too
    opt.note_replayed()
    assert opt.state[w]["step"] == 2 and opt.state[b]["step"] == 2
    # under a schedule the host mirror follows the table, group by group
    ds = S.DeviceSchedule(opt, S.wsd_lambda(9, 4, 3), 9)
    assert ds.base_lrs == [2e-3, 1e-4]
    opt.attach_schedule(ds)
    opt.note_replayed()
    assert [g["lr"] for g in opt.param_groups] == [ds.host_lr(0, 2), ds.host_lr(1, 2)]
    assert opt.param_groups[0]["lr"] == float(np.float32(2e-3 * 0.75))
    with pytest.raises(ValueError):
        optim.Muon([torch.nn.Parameter(torch.zeros(2, 2))]).attach_schedule(ds)
