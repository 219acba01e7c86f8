"""CPU restatement of the reference's ``LitParadis.on_before_optimizer_step`` (trainer.py:844-923), line by line, for the
tests: the Lightning module cannot be imported here, so only its arithmetic is written again, in new code.

``metrics(named, grads, exp_avgs, dtype)``: ``named`` is a list of ``(name, tensor)`` with names as ``LitParadis`` sees
them (``"model.<submodule>. ..."``: the group key is ``name.split(".")[1]``); ``grads[i]`` is the gradient of tensor i
or ``None``; ``exp_avgs[i]`` is ``optimizer.state[p]["exp_avg"]`` or ``None`` where the optimiser keeps no such entry.
Evaluated in fp64 it is the reference value; in fp32 it follows the reference's operation order (per tensor a square or
product and ``.sum()``, then scalar adds) and gives fp32's own error.  ``seq=True`` replaces every ``.sum()`` by a
strictly sequential accumulation in the working dtype (numpy.cumsum), the least favourable ordinary order.

Returns ``(logged, sums)``: ``logged`` holds exactly the keys the reference hands to ``log_dict``; ``sums`` holds, per
group key and under ``"total"``, the tuple ``(sum p^2, sum g^2, sum g.m, sum m^2)`` the logged values are formed from
(for every group, with or without gradients)."""
from collections import defaultdict

import numpy as np
import torch


def _sum(t, seq):
    if not seq:
        return t.sum()
    a = np.ascontiguousarray(t.detach().reshape(-1).numpy())
    if a.size == 0:
        return torch.zeros((), dtype=t.dtype)
    return torch.tensor(np.cumsum(a, dtype=a.dtype)[-1], dtype=t.dtype)


def metrics(named, grads, exp_avgs, dtype=torch.float64, seq=False):
    zero = lambda: torch.zeros((), dtype=dtype)      # noqa: E731
    grad_sq, param_sq = defaultdict(zero), defaultdict(zero)
    momentum_sq, dot_product_total = defaultdict(zero), defaultdict(zero)
    for (name, p), grad, exp_avg in zip(named, grads, exp_avgs):
        if p is None:
            continue
        key = name.split(".")[1]
        param_sq[key] = param_sq[key] + _sum(p.detach().to(dtype) ** 2, seq)
        if grad is not None:
            g = grad.detach().to(dtype)
            grad_sq[key] = grad_sq[key] + _sum(g ** 2, seq)
            if exp_avg is not None:
                m = exp_avg.detach().to(dtype)
                dot_product_total[key] = dot_product_total[key] + _sum(g * m, seq)
                momentum_sq[key] = momentum_sq[key] + _sum(m ** 2, seq)
    total_grad = torch.stack(list(grad_sq.values()) or [zero()]).sum().sqrt()
    logged = {"grad/total": total_grad}
    eps = 1e-12
    total_dot, total_grad_sq, total_momentum_sq = zero(), zero(), zero()
    for k in sorted(grad_sq.keys()):
        gnorm = grad_sq[k].sqrt()
        pnorm = param_sq[k].sqrt().clamp_min(eps)
        logged[f"grad/{k}"] = gnorm
        logged[f"gradratio/{k}"] = gnorm / pnorm
        logged[f"pnorm/{k}"] = pnorm
        if momentum_sq[k] > 0:
            g_norm = grad_sq[k].sqrt()
            m_norm = momentum_sq[k].sqrt()
            logged[f"grad_alignment/{k}"] = dot_product_total[k] / (g_norm * m_norm + eps)
        total_dot = total_dot + dot_product_total[k]
        total_grad_sq = total_grad_sq + grad_sq[k]
        total_momentum_sq = total_momentum_sq + momentum_sq[k]
    if total_momentum_sq > 0:
        logged["grad_alignment/total"] = total_dot / (total_grad_sq.sqrt() * total_momentum_sq.sqrt() + eps)
    sums = {}
    total_param_sq = zero()
    for k in sorted(param_sq.keys()):
        total_param_sq = total_param_sq + param_sq[k]
        sums[k] = tuple(float(d[k]) if k in d else 0.0 for d in (param_sq, grad_sq, dot_product_total, momentum_sq))
    sums["total"] = (float(total_param_sq), float(total_grad_sq), float(total_dot), float(total_momentum_sq))
    return {k: float(v) for k, v in logged.items()}, sums
