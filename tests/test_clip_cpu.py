"""CPU: the host side of gradient accumulation and global-norm clipping - the C-ABI symbols of ``csrc/clip.hip`` and their
argument rejection before any HIP call, and the gating of ``harness.TrainStep`` (reference trainer.py:498-587: zero on the
first batch of a window, loss / (S N), optimiser and scheduler on the last batch or on ``is_last_batch``; train.py:52-53:
clip between the last backward and the optimiser step) against a hand-written loop of ``zero_grad`` / ``rollout_loss`` /
``torch.nn.utils.clip_grad_norm_`` / ``torch.optim.AdamW.step`` on a stub model, to ``torch.equal`` precision."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

from paradis_model_amd.config import default_config
from paradis_model_amd.harness import TrainStep, rollout_loss, synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("paradis_clip_grad_chunk", "paradis_clip_grad_ws_bytes", "paradis_clip_grad_norm")


# ================================================================================================ the C ABI
def test_clip_symbols_are_declared_exported_and_bound():
    from paradis_model_amd import _lib
    with open(os.path.join(ROOT, "include", "paradis_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "ABI 10, additive" in header
    assert len(_lib.SIGNATURES["paradis_clip_grad_norm"][1]) == 10
    assert _lib.SIGNATURES["paradis_clip_grad_norm"][1][6] is ctypes.c_double
    L = _lib.lib
    assert L.paradis_abi_version() == 10
    C = L.paradis_clip_grad_chunk()
    assert C >= 1024 and C % 4 == 0
    assert L.paradis_clip_grad_ws_bytes(0) == 0
    assert L.paradis_clip_grad_ws_bytes(-1) == 0
    for n in (1, 7, 3000):
        assert L.paradis_clip_grad_ws_bytes(n) >= 8 * n


def test_clip_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first

    def call(grads=fake, numel=fake, ct=fake, co=fake, T=2, chunks=3, max_norm=1.0, ws=fake, out=fake):
        return L.paradis_clip_grad_norm(grads, numel, ct, co, T, chunks, max_norm, ws, out, None)

    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(max_norm=bad) == 1 and "max_norm" in _lib.last_error(), bad
        assert call(max_norm=bad, chunks=0) == 1 and "max_norm" in _lib.last_error(), bad
    for kw in (dict(T=-1), dict(chunks=-1)):
        assert call(**kw) == 1 and "counts" in _lib.last_error()
    for kw in (dict(grads=None), dict(numel=None), dict(ct=None), dict(co=None)):
        assert call(**kw) == 1 and "tables" in _lib.last_error()
    assert call(out=None) == 1 and "result" in _lib.last_error()
    assert call(ws=None) == 1 and "workspace" in _lib.last_error()
    assert call(T=0) == 1 and "no tensor" in _lib.last_error()


def test_clip_grad_norm_host_checks_and_cpu_fallback():
    from paradis_model_amd import clip
    w = nn.Parameter(torch.tensor([3.0, 4.0]))
    v = nn.Parameter(torch.tensor([1.0]))             # no gradient: skipped
    w.grad = torch.tensor([6.0, 8.0])
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_norm"):
            clip.clip_grad_norm_([w, v], bad)
    out = clip.clip_grad_norm_([w, v], 5.0)
    assert out.shape == (2,) and out.dtype == torch.float32
    assert float(out[0]) == 10.0 and abs(float(out[1]) - 0.5) <= 1e-7
    assert torch.allclose(w.grad, torch.tensor([3.0, 4.0]), rtol=1e-6) and v.grad is None
    out = clip.clip_grad_norm_(w, 50.0)               # a single tensor; nothing to clip
    assert float(out[1]) == 1.0 and abs(float(out[0]) - 5.0) <= 1e-6
    assert tuple(clip.clip_grad_norm_([], 1.0).tolist()) == (0.0, 1.0)


# ================================================================================================ the training step
H, W, B, S = 8, 16, 2, 3


def _mse(out, target):
    return (out - target).square().mean()


def _model():
    torch.manual_seed(0)
    return nn.Conv2d(186, 97, 1)


def _cfg(**training):
    cfg = default_config()
    for k, v in training.items():
        if k == "detach_gradient_every":
            cfg.training.optimizer[k] = v
        else:
            cfg.training[k] = v
    return cfg


@pytest.fixture(scope="module")
def batches():
    return [synthetic_batch(H, W, False, B, S, seed=100 + i) for i in range(7)]


def _hand_loop(cfg, batches, N, clip_val, detach=None, flush=True, lr_of_step=None):
    """the reference's manual optimisation, written out: (parameters, losses as rollout_loss returns them, optimiser steps)"""
    model = _model()
    o = cfg.training.optimizer
    opt = torch.optim.AdamW(model.parameters(), lr=o.lr, weight_decay=o.weight_decay, betas=(o.beta1, o.beta2))
    losses, steps = [], 0

    def optimizer_step():
        nonlocal steps
        if clip_val:
            torch.nn.utils.clip_grad_norm_(list(model.parameters()), clip_val)
        if lr_of_step is not None:
            for group in opt.param_groups:
                group["lr"] = lr_of_step(steps)
        opt.step()
        steps += 1

    for k, batch in enumerate(batches):
        if k % N == 0:
            opt.zero_grad(set_to_none=True)
        loss, _ = rollout_loss(model, _mse, batch, num_common=83, n_inputs=2, accum=N, detach_every=detach)
        losses.append(loss)
        if (k + 1) % N == 0:
            optimizer_step()
    if flush and len(batches) % N:
        optimizer_step()
    return model, losses, steps


def _same_parameters(a, b):
    return all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_default_step_is_the_plain_loop(batches):
    cfg = _cfg()
    model = _model()
    step = TrainStep(model, _mse, cfg)
    assert step.accumulate == 1 and step.clip_val is None
    losses = [step(b) for b in batches[:3]]
    ref, ref_losses, n = _hand_loop(cfg, batches[:3], 1, None)
    assert _same_parameters(model, ref) and step.opt_steps == n == 3
    assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses))
    assert step.last_grad_norm is None and step.pending == 0 and step.flush() is False


@pytest.mark.parametrize("clip_val", [None, 0.05])
def test_window_of_three_over_seven_calls_and_flush(batches, clip_val):
    base = 5e-4
    lam = lambda k: 1.0 / (k + 1)                                   # noqa: E731
    cfg = _cfg()
    model = _model()
    step = TrainStep(model, _mse, cfg, accumulate_grad_batches=3, gradient_clip_val=clip_val, schedule=(lam, 10))
    pend, losses = [], []
    for b in batches:
        losses.append(step(b))
        pend.append(step.pending)
    assert pend == [1, 2, 0, 1, 2, 0, 1] and step.opt_steps == 2
    assert step.flush() is True and step.pending == 0 and step.opt_steps == 3
    assert step.flush() is False and step.opt_steps == 3
    lr32 = lambda k: float(np.float32(base * lam(k)))               # noqa: E731
    ref, ref_losses, n = _hand_loop(cfg, batches, 3, clip_val, lr_of_step=lr32)
    assert n == 3 and _same_parameters(model, ref)
    # the host schedule advanced three times, not seven: the last step ran at the learning rate of step index 2
    assert step.opt.param_groups[0]["lr"] == lr32(2) != lr32(6)
    # the returned loss is the rollout mean of the batch, without the 1/N that the accumulated loss carries
    for got, acc, b in zip(losses, ref_losses, batches):
        assert abs(float(got) - 3.0 * float(acc)) <= 1e-6 * abs(float(got))
    if clip_val is None:
        assert step.last_grad_norm is None
    else:
        norm, coef = step.last_grad_norm.tolist()
        assert norm > clip_val and 0.0 < coef < 1.0                 # the clip did bite (else the case shows nothing)


def test_returned_loss_is_the_plain_rollout_mean(batches):
    model = _model()
    step = TrainStep(model, _mse, _cfg(), accumulate_grad_batches=4)
    got = float(step(batches[0]))
    plain, _ = rollout_loss(_model(), _mse, batches[0], num_common=83, n_inputs=2, backward=False)
    assert abs(got - float(plain)) <= 1e-6 * abs(got)


def test_clipping_on_off_and_zero_is_off(batches):
    cfg = _cfg()
    runs = {}
    for name, val in (("off", None), ("zero", 0), ("zero_f", 0.0), ("on", 0.05), ("loose", 1e9)):
        model = _model()
        step = TrainStep(model, _mse, cfg, gradient_clip_val=val)
        for b in batches[:3]:
            step(b)
        runs[name] = (model, step)
    for name in ("zero", "zero_f"):
        assert runs[name][1].clip_val is None and runs[name][1].last_grad_norm is None
        assert _same_parameters(runs[name][0], runs["off"][0])
    ref, _, _ = _hand_loop(cfg, batches[:3], 1, 0.05)
    assert _same_parameters(runs["on"][0], ref)
    assert not _same_parameters(runs["on"][0], runs["off"][0])
    assert float(runs["on"][1].last_grad_norm[1]) < 1.0
    assert _same_parameters(runs["loose"][0], runs["off"][0]) and float(runs["loose"][1].last_grad_norm[1]) == 1.0
    # the values come from the configuration when the keywords are not given
    cfg2 = _cfg(gradient_clip_val=0.05, accumulate_grad_batches=2)
    step = TrainStep(_model(), _mse, cfg2)
    assert step.clip_val == 0.05 and step.accumulate == 2
    assert TrainStep(_model(), _mse, cfg2, accumulate_grad_batches=1, gradient_clip_val=0).clip_val is None


def test_detach_gradient_every_one_with_window_and_clip(batches):
    cfg = _cfg(detach_gradient_every=1)
    model = _model()
    step = TrainStep(model, _mse, cfg, accumulate_grad_batches=2, gradient_clip_val=0.05)
    assert step.detach_every == 1
    for b in batches[:4]:
        step(b)
    ref, _, n = _hand_loop(cfg, batches[:4], 2, 0.05, detach=1)
    assert n == step.opt_steps == 2 and _same_parameters(model, ref)
    full, _, _ = _hand_loop(cfg, batches[:4], 2, 0.05, detach=None)
    assert not _same_parameters(model, full)                        # the truncation is visible at this size


def test_window_needs_a_whole_window_and_nothing_pending(batches):
    step = TrainStep(_model(), _mse, _cfg(), accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="batches"):
        step.window(batches[:3])
    losses = step.window(batches[:2])
    assert losses.shape == (2,) and step.pending == 0 and step.opt_steps == 1
    step(batches[0])
    with pytest.raises(ValueError, match="pending"):
        step.window(batches[:2])


def test_refusals(batches, monkeypatch):
    cfg = _cfg()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gradient_clip_val"):
            TrainStep(_model(), _mse, cfg, gradient_clip_val=bad)
    for bad in (0, -2, 1.5, "2", True):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            TrainStep(_model(), _mse, cfg, accumulate_grad_batches=bad)
    with pytest.raises(ValueError, match="stats"):
        TrainStep(_model(), _mse, cfg, accumulate_grad_batches=2, stats=object())
    # the weight-gradient side stream hands gradients over safely only while .grad is None
    monkeypatch.setenv("PARADIS_WGRAD_STREAM", "1")
    ops = sys.modules.get("paradis_model_amd.ops")
    if ops is not None:
        monkeypatch.setattr(ops.WgradSide, "enabled", True)
    with pytest.raises(ValueError, match="PARADIS_WGRAD_STREAM"):
        TrainStep(_model(), _mse, cfg, accumulate_grad_batches=2)
    TrainStep(_model(), _mse, cfg, accumulate_grad_batches=1)       # N = 1 stays allowed with the side stream
