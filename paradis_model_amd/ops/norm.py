"""a8 ChannelNorm (reference model/blocks.py:118-134), optionally over a virtual concat; csrc/norm.hip"""
import torch

from .._lib import check, dptr, lib, stream_ptr
from ._core import (GEMM_BF16, OPS, RAW, _autograd, _cotangent, _define, _eager_forward, _f32, _f32_or_bf16, _fake, _is16,
                    _plain, _plane_view, _want_bf16_out, _ws, require_hip)


@_define("channel_norm(Tensor x1, Tensor? x2, Tensor weight, Tensor bias, float eps, bool out_bf16=False) "
         "-> (Tensor, Tensor, Tensor)")
def _channel_norm(x1, x2, weight, bias, eps, out_bf16=False):
    """``out_bf16``: y as a bf16 tensor (bf16-mixed mode, consumer = a pointwise GEMM: the reference casts the norm's fp32
    output to bf16 at that conv2d, model/blocks.py:86 under train.py:56); mean / rstd stay fp32."""
    _f32(x1, x2, weight, bias)
    x1, bs1 = _plane_view(x1)
    B, C1, H, W = x1.shape
    C2, bs2 = 0, 0
    if x2 is not None:
        x2, bs2 = _plane_view(x2)
        C2 = x2.shape[1]
    P = H * W
    y = torch.empty(B, C1 + C2, H, W, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x1.device)
    mean = torch.empty(B, P, dtype=x1.dtype, device=x1.device)
    rstd = torch.empty_like(mean)
    fn = lib.paradis_channel_norm_fwd16 if out_bf16 else lib.paradis_channel_norm_fwd
    check(fn(dptr(x1), dptr(x2), dptr(weight), dptr(bias), dptr(y), dptr(mean),
             dptr(rstd), B, C1, C2, P, bs1, bs2, eps, stream_ptr()), "channel_norm_fwd")
    return y, mean, rstd


@_fake("channel_norm")
def _(x1, x2, weight, bias, eps, out_bf16=False):
    B, C1, H, W = x1.shape
    C = C1 + (x2.shape[1] if x2 is not None else 0)
    return (x1.new_empty(B, C, H, W, dtype=torch.bfloat16 if out_bf16 else torch.float32), x1.new_empty(B, H * W),
            x1.new_empty(B, H * W))


@_define("channel_norm_backward(Tensor gy, Tensor x1, Tensor? x2, Tensor weight, Tensor mean, Tensor rstd, "
         "Tensor? add) -> (Tensor, Tensor, Tensor, Tensor)")
def _channel_norm_backward(gy, x1, x2, weight, mean, rstd, add):
    """``add``: a gradient that reaches x1 along another path (the residual branch around the block);
    it is added inside the kernel instead of by a separate accumulation pass."""
    _f32(x1, x2, add)
    _f32_or_bf16(GEMM_BF16, gy)
    x1, bs1 = _plane_view(x1)
    B, C1, H, W = x1.shape
    C2, bs2 = 0, 0
    if x2 is not None:
        x2, bs2 = _plane_view(x2)
        C2 = x2.shape[1]
    P, C = H * W, C1 + C2
    gy = gy.contiguous()
    add_bs = 0
    if add is not None:
        add, add_bs = _plane_view(add)
    if _is16(gy) and not lib.paradis_channel_norm_bwd16_ok(B, C, P):
        gy = gy.float().contiguous()        # (a bf16 cotangent is read as stored by the streaming kernels only)
    gx1 = torch.empty(B, C1, H, W, dtype=x1.dtype, device=gy.device)
    gx2 = torch.empty(B, C2, H, W, dtype=x1.dtype, device=gy.device)
    gw = torch.empty(C, dtype=x1.dtype, device=gy.device)
    gb = torch.empty_like(gw)
    ws = _ws(lib.paradis_channel_norm_bwd_ws_bytes(B, C, P), gy.device)
    fn = lib.paradis_channel_norm_bwd16 if _is16(gy) else lib.paradis_channel_norm_bwd
    check(fn(dptr(gy), dptr(x1), dptr(x2) if C2 else None, dptr(weight), dptr(mean),
             dptr(rstd), dptr(gx1), dptr(gx2) if C2 else None, dptr(gw), dptr(gb), B,
             C1, C2, P, bs1, bs2, C1 * P, C2 * P, dptr(add), add_bs, dptr(ws),
             stream_ptr()), "channel_norm_bwd")
    return gx1, gx2, gw, gb


@_fake("channel_norm_backward")
def _(gy, x1, x2, weight, mean, rstd, add):
    B, C1, H, W = x1.shape
    C2 = x2.shape[1] if x2 is not None else 0
    return (x1.new_empty(B, C1, H, W), x1.new_empty(B, C2, H, W), x1.new_empty(C1 + C2), x1.new_empty(C1 + C2))


def _norm_setup(ctx, inputs, output):
    x1, x2, weight, bias, eps = inputs[:5]
    y, mean, rstd = output
    ctx.save_for_backward(x1, x2, weight, mean, rstd)
    ctx.mark_non_differentiable(mean, rstd)
    ctx.set_materialize_grads(False)


def _norm_backward(ctx, gy, gmean=None, grstd=None):
    x1, x2, weight, mean, rstd = ctx.saved_tensors
    if gy is None:
        return None, None, None, None, None, None
    gx1, gx2, gw, gb = _channel_norm_backward(_cotangent(gy, True), x1, x2, weight, mean, rstd, None)
    return gx1, (gx2 if x2 is not None else None), gw, gb, None, None


_autograd("channel_norm", _norm_setup, _norm_backward)


class _ChannelNormSkip(torch.autograd.Function):
    """``(channel_norm(x), x)``: the second output is ``x`` itself for the residual branch around the
    block, so every gradient of ``x`` arrives at this node and is added inside the backward kernel
    (``channel_norm_backward(..., add=...)``) instead of by autograd's accumulation pass.  Eager only:
    under ``torch.compile`` the plain op is used and the traced graph holds the addition."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, eps, out_bf16):
        y, mean, rstd = _eager_forward("channel_norm", (x1, x2, weight, bias, eps, out_bf16))
        ctx.save_for_backward(x1, x2, weight, mean, rstd)
        ctx.set_materialize_grads(False)
        return y, x1

    @staticmethod
    def backward(ctx, gy, gskip):
        x1, x2, weight, mean, rstd = ctx.saved_tensors
        if gy is None:          # only the skip path was used
            return gskip, None, None, None, None, None
        gy = _cotangent(gy, True)
        K = RAW if _plain(gy) else OPS
        gx1, gx2, gw, gb = K["channel_norm_backward"](gy, x1, x2, weight, mean, rstd, gskip)
        return gx1, (gx2 if x2 is not None else None), gw, gb, None, None


def channel_norm(x, weight, bias, eps: float = 1e-5, x_extra=None, out_bf16: bool = False):
    """ChannelNorm over channels of ``x`` (and, virtually concatenated after them, ``x_extra``).
    ``out_bf16``: a request (see ``_want_bf16_out``) - the output as a bf16 tensor for a pointwise consumer."""
    require_hip(x, x_extra, weight, bias)
    return _channel_norm(x, x_extra, weight, bias, float(eps), _want_bf16_out(x, out_bf16))[0]


def channel_norm_skip(x, weight, bias, eps: float = 1e-5, x_extra=None, out_bf16: bool = False):
    """``(channel_norm(x), x)`` for a block with a residual branch around it (see ``_ChannelNormSkip``)."""
    require_hip(x, x_extra, weight, bias)
    if torch.compiler.is_compiling():
        return _channel_norm(x, x_extra, weight, bias, float(eps))[0], x
    return _ChannelNormSkip.apply(x, x_extra, weight, bias, float(eps), _want_bf16_out(x, out_bf16))
