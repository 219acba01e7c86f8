"""a1 geocyclic padding (reference model/padding.py:11-39); csrc/pad.hip"""
import torch
from torch import Tensor

from .._lib import check, dptr, lib, stream_ptr
from ._core import _autograd, _define, _f32, _fake, _planes_hw, require_hip


@_define("geocyclic_pad(Tensor x, int p) -> Tensor")
def _geocyclic_pad(x, p):
    _f32(x)
    x = x.contiguous()
    planes, H, W = _planes_hw(x)
    y = torch.empty(*x.shape[:-2], H + 2 * p, W + 2 * p, dtype=x.dtype, device=x.device)
    check(lib.paradis_geocyclic_pad_fwd(dptr(x), dptr(y), planes, H, W, p, stream_ptr()), "geocyclic_pad_fwd")
    return y


@_fake("geocyclic_pad")
def _(x, p):
    return x.new_empty(*x.shape[:-2], x.shape[-2] + 2 * p, x.shape[-1] + 2 * p)


@_define("geocyclic_pad_backward(Tensor gy, int p) -> Tensor")
def _geocyclic_pad_backward(gy, p):
    _f32(gy)
    gy = gy.contiguous()
    H, W = gy.shape[-2] - 2 * p, gy.shape[-1] - 2 * p
    gx = torch.empty(*gy.shape[:-2], H, W, dtype=gy.dtype, device=gy.device)
    check(lib.paradis_geocyclic_pad_bwd(dptr(gy), dptr(gx), gx.numel() // (H * W), H, W, p, stream_ptr()),
          "geocyclic_pad_bwd")
    return gx


@_fake("geocyclic_pad_backward")
def _(gy, p):
    return gy.new_empty(*gy.shape[:-2], gy.shape[-2] - 2 * p, gy.shape[-1] - 2 * p)


def _pad_setup(ctx, inputs, output):
    ctx.p = inputs[1]


def _pad_backward(ctx, gy):
    return _geocyclic_pad_backward(gy, ctx.p), None


_autograd("geocyclic_pad", _pad_setup, _pad_backward)


def geocyclic_pad(x: Tensor, p: int) -> Tensor:
    if p == 0:
        return x
    assert x.dim() == 4, "Input must be 4-dimensional [batch, channels, lat, lon]"
    assert x.shape[-1] % 2 == 0, "Number of longitude points must be even"
    require_hip(x)
    return _geocyclic_pad(x, int(p))
