"""rows f1-f2: loss and rollout glue - the weighted pointwise loss and the AMSE spectral loss;
csrc/train.hip, csrc/sht.hip"""
from typing import Tuple

import torch
from torch import Tensor

from .._lib import check, dptr, lib, stream_ptr
from ._core import _autograd, _define, _f32, _fake, _ws, require_hip
from .elementwise import _scale


@_define("paradis_loss(Tensor pred, Tensor target, Tensor wf, Tensor? wl, int kind, float delta, bool want_grad) "
         "-> (Tensor, Tensor)")
def _paradis_loss(pred, target, wf, wl, kind, delta, want_grad):
    """mean(wf[c] * wl[h] * l(pred - target)) and, in the same pass, its derivative w.r.t. pred."""
    _f32(pred, target, wf, wl)
    pred, target = pred.contiguous(), target.contiguous()
    B, C, H, W = pred.shape
    assert target.shape == pred.shape and wf.numel() == C and (wl is None or wl.numel() == H)
    loss = torch.empty((), dtype=pred.dtype, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else pred.new_empty(0)
    partial = torch.empty(lib.paradis_loss_blocks(pred.numel()), dtype=pred.dtype, device=pred.device)
    check(lib.paradis_loss_fwd_bwd(dptr(pred), dptr(target), dptr(wf), dptr(wl), dptr(loss),
                                   dptr(grad) if want_grad else None, dptr(partial), B, C, H, W, kind, delta,
                                   stream_ptr()), "loss_fwd_bwd")
    return loss, grad


@_fake("paradis_loss")
def _(pred, target, wf, wl, kind, delta, want_grad):
    return pred.new_empty(()), (pred.new_empty(pred.shape) if want_grad else pred.new_empty(0))


def _loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)


def _loss_backward(ctx, gout, ggrad=None):
    (grad,) = ctx.saved_tensors
    if gout is None:
        return (None,) * 7
    if grad.numel() == 0:
        raise RuntimeError("paradis_loss was called with want_grad=False but its gradient is requested")
    return (_scale(grad, gout),) + (None,) * 6


_autograd("paradis_loss", _loss_setup, _loss_backward)


def paradis_loss(pred, target, feature_weights, lat_weights=None, kind="reversed_huber", delta=1.0):
    """mean(feature_weights[c] * lat_weights[h] * l(pred - target)); forward and d/dpred in one pass."""
    code = {"mse": 0, "reversed_huber": 1}[kind]
    require_hip(pred, target, feature_weights, lat_weights)
    want_grad = torch.is_grad_enabled() and pred.requires_grad
    return _paradis_loss(pred, target, feature_weights, lat_weights, code, float(delta), want_grad)[0]


# ---------------------------------------------------------------------------
# row f1 (AMSE): the spectral loss of reference utils/amse_loss.py (sht.hip)
# ---------------------------------------------------------------------------
def amse_grid_check(H: int, W: int) -> None:
    """the reference builds its transform for W = 2(H-1) only (utils/loss.py:93, an equiangular grid with both poles)"""
    if H < 3 or W != 2 * (H - 1):
        raise ValueError(f"amse: the equiangular spherical-harmonic transform needs nlon = 2*(nlat-1) "
                         f"(a latitude grid with both poles), got nlat={H}, nlon={W}")


@_define("amse_tables(Tensor like, int nlat, int nlon) -> (Tensor, Tensor)", autocast=False)
def _amse_tables(like, nlat, nlon):
    """(Legendre x quadrature table [tri(nlat-1) * nlat], twiddle table [nlon, 2*(nlat-1)]) on like's device"""
    amse_grid_check(nlat, nlon)
    leg = torch.empty(lib.paradis_amse_table_floats(nlat), dtype=torch.float32, device=like.device)
    tw = torch.empty(nlon, 2 * (nlat - 1), dtype=torch.float32, device=like.device)
    ws = _ws(lib.paradis_amse_tables_ws_bytes(nlat), like.device)
    check(lib.paradis_amse_tables(dptr(leg), dptr(tw), dptr(ws), nlat, nlon, stream_ptr()), "amse_tables")
    return leg, tw


@_fake("amse_tables")
def _(like, nlat, nlon):
    M = nlat - 1
    return like.new_empty(M * (M + 1) // 2 * nlat, dtype=torch.float32), like.new_empty(nlon, 2 * M, dtype=torch.float32)


@_define("amse_loss(Tensor pred, Tensor target, Tensor leg, Tensor twiddle, bool want_grad) -> (Tensor, Tensor)")
def _amse_loss(pred, target, leg, twiddle, want_grad):
    """AMSE(pred, target) over the [B, C] planes and, in the same launch sequence, its derivative w.r.t. pred."""
    _f32(pred, target, leg, twiddle)
    pred, target = pred.contiguous(), target.contiguous()
    B, C, H, W = pred.shape
    assert target.shape == pred.shape
    N = B * C
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else pred.new_empty(0)
    ws = _ws(lib.paradis_amse_ws_bytes(N, H), pred.device)
    check(lib.paradis_amse_loss(dptr(pred) if N else None, dptr(target) if N else None, dptr(leg), dptr(twiddle),
                                dptr(loss), dptr(grad) if (want_grad and N) else None, dptr(ws), N, H, W, stream_ptr()),
          "amse_loss")
    return loss, grad


@_fake("amse_loss")
def _(pred, target, leg, twiddle, want_grad):
    return pred.new_empty(()), (pred.new_empty(pred.shape) if want_grad else pred.new_empty(0))


def _amse_backward(ctx, gout, ggrad=None):
    (grad,) = ctx.saved_tensors
    if gout is None:
        return (None,) * 5
    if grad.numel() == 0 and grad.dim() == 1:
        raise RuntimeError("amse_loss was called with want_grad=False but its gradient is requested")
    return (_scale(grad, gout),) + (None,) * 4


_autograd("amse_loss", _loss_setup, _amse_backward)     # (the same pair of outputs as ``paradis_loss``)

_AMSE_TABLES = {}


def amse_tables(nlat: int, nlon: int, device) -> Tuple[Tensor, Tensor]:
    """The cached tables of one grid on one device, built on the first eager call (never inside a graph capture: the
    warm-up steps of harness.GraphedTrainStep run eagerly first)."""
    device = torch.device(device)
    live = device.type == "cuda" and torch.cuda.is_available()
    index = device.index if device.index is not None else (torch.cuda.current_device() if live else 0)
    key = (int(nlat), int(nlon), device.type, index)
    t = _AMSE_TABLES.get(key)
    if t is not None:
        return t
    if live and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("amse_loss: the spherical-harmonic tables of this grid are not built yet; run one eager "
                           "call before capturing a graph")
    with torch.inference_mode(False), torch.no_grad():
        t = _amse_tables(torch.empty(0, device=device), int(nlat), int(nlon))
    # only tables made by an eager call are cached (a traced call can return fakes without storage)
    if all(type(x) is Tensor for x in t) and not torch.compiler.is_compiling():
        _AMSE_TABLES[key] = t
    return t


def amse_loss(pred: Tensor, target: Tensor) -> Tensor:
    """Scalar AMSE of reference ``AMSELoss(nlat=H, nlon=2(H-1), grid="equiangular")`` (utils/amse_loss.py), unweighted:
    both inputs widened to fp32, spherical-harmonic transforms, per-scale amplitude + decorrelation terms, mean over
    scales and (b, c); a NaN result becomes 1e6 (with a zero gradient).  The target gets no gradient."""
    if pred.dim() != 4 or target.shape != pred.shape:
        raise ValueError(f"amse_loss: pred and target must be [B, C, H, W] of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    H, W = pred.shape[-2:]
    amse_grid_check(H, W)
    require_hip(pred, target)
    pred, target = pred.float(), target.float().detach()
    leg, tw = amse_tables(H, W, pred.device)
    want_grad = torch.is_grad_enabled() and pred.requires_grad
    return _amse_loss(pred, target, leg, tw, want_grad)[0]
