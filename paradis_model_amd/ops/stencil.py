"""a7 depthwise stencil on the virtual geocyclic halo (reference model/blocks.py:101-113); csrc/stencil*.hip"""
import torch

from .._lib import check, dptr, lib, stream_ptr
from ._core import (GEMM_BF16, OPS, RAW, _autograd, _cotangent, _define, _eager_forward, _f32, _f32_or_bf16, _fake, _is16,
                    _plain, _want_bf16_out, _ws, require_hip)


@_define("dwconv_geo(Tensor x, Tensor weight, Tensor? bias, bool out_bf16=False) -> Tensor")
def _dwconv_geo(x, weight, bias, out_bf16=False):
    """``out_bf16``: y as a bf16 tensor (bf16-mixed mode: the consumer is the SepConv's pointwise GEMM, which rounds its
    operand to bf16 anyway - reference model/blocks.py:107-110 under autocast)."""
    _f32(x, weight, bias)
    x = x.contiguous()
    B, C, H, W = x.shape
    k = weight.shape[-1]
    assert weight.shape == (C, 1, k, k), "depthwise weight must be [C,1,k,k]"
    w = weight.contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    fn = lib.paradis_dwconv_geo_fwd16 if out_bf16 else lib.paradis_dwconv_geo_fwd
    check(fn(dptr(x), dptr(w), dptr(bias), dptr(y), B, C, H, W, k, stream_ptr()), "dwconv_geo_fwd")
    return y


@_fake("dwconv_geo")
def _(x, weight, bias, out_bf16=False):
    return x.new_empty(x.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32)


@_define("dwconv_geo_dgrad(Tensor gy, Tensor weight) -> Tensor")
def _dwconv_geo_dgrad(gy, weight):
    _f32(gy, weight)
    gy, w = gy.contiguous(), weight.contiguous()
    B, C, H, W = gy.shape
    gx = torch.empty_like(gy)
    check(lib.paradis_dwconv_geo_dgrad(dptr(gy), dptr(w), dptr(gx), B, C, H, W, w.shape[-1], stream_ptr()),
          "dwconv_geo_dgrad")
    return gx


@_fake("dwconv_geo_dgrad")
def _(gy, weight):
    return gy.new_empty(gy.shape)


@_define("dwconv_geo_dgrad_add(Tensor gy, Tensor weight, Tensor addend) -> Tensor")
def _dwconv_geo_dgrad_add(gy, weight, addend):
    _f32(gy, weight, addend)
    gy, w, addend = gy.contiguous(), weight.contiguous(), addend.contiguous()
    assert addend.shape == gy.shape
    B, C, H, W = gy.shape
    gx = torch.empty_like(gy)
    check(lib.paradis_dwconv_geo_dgrad_add(dptr(gy), dptr(w), dptr(addend), dptr(gx), B, C, H, W, w.shape[-1],
                                           stream_ptr()), "dwconv_geo_dgrad_add")
    return gx


@_fake("dwconv_geo_dgrad_add")
def _(gy, weight, addend):
    return gy.new_empty(gy.shape)


@_define("dwconv_geo_wgrad(Tensor gy, Tensor x, int k, bool has_bias) -> (Tensor, Tensor)")
def _dwconv_geo_wgrad(gy, x, k, has_bias):
    _f32(gy, x)
    gy, x = gy.contiguous(), x.contiguous()
    B, C, H, W = x.shape
    gw = torch.empty(C, 1, k, k, dtype=x.dtype, device=x.device)
    gb = torch.empty(C if has_bias else 0, dtype=x.dtype, device=x.device)
    ws = _ws(lib.paradis_dwconv_geo_wgrad_ws_bytes(B, C, H, W, k), x.device)
    check(lib.paradis_dwconv_geo_wgrad(dptr(gy), dptr(x), dptr(gw), dptr(gb) if has_bias else None, B, C, H, W, k,
                                       dptr(ws), stream_ptr()), "dwconv_geo_wgrad")
    return gw, gb


@_fake("dwconv_geo_wgrad")
def _(gy, x, k, has_bias):
    C = x.shape[1]
    return x.new_empty(C, 1, k, k), x.new_empty(C if has_bias else 0)


@_define("dwconv_geo_bwd(Tensor gy, Tensor x, Tensor weight, Tensor? addend, bool has_bias) -> (Tensor, Tensor, Tensor)")
def _dwconv_geo_bwd(gy, x, weight, addend, has_bias):
    """(gx (+ addend), gw, gb) of the stencil in one call: with k = 5 on the reference grids one kernel that reads gy
    once (paradis_dwconv_geo_bwd); bit-identical to ``dwconv_geo_dgrad`` (``_add``) + ``dwconv_geo_wgrad``."""
    _f32(x, weight, addend)
    _f32_or_bf16(GEMM_BF16, gy)
    B, C, H, W = x.shape
    k = weight.shape[-1]
    if _is16(gy) and not lib.paradis_dwconv_geo_bwd16_ok(H, W, k):
        gy = gy.float()             # (a bf16 cotangent is read as stored on the whole-plane grids only)
    gy, x, w = gy.contiguous(), x.contiguous(), weight.contiguous()
    if addend is not None:
        addend = addend.contiguous()
        assert addend.shape == gy.shape
    gx = torch.empty(gy.shape, dtype=x.dtype, device=x.device)
    gw = torch.empty(C, 1, k, k, dtype=x.dtype, device=x.device)
    gb = torch.empty(C if has_bias else 0, dtype=x.dtype, device=x.device)
    ws = _ws(lib.paradis_dwconv_geo_wgrad_ws_bytes(B, C, H, W, k), x.device)
    fn = lib.paradis_dwconv_geo_bwd16 if _is16(gy) else lib.paradis_dwconv_geo_bwd
    check(fn(dptr(gy), dptr(x), dptr(w), dptr(addend), dptr(gx), dptr(gw),
             dptr(gb) if has_bias else None, B, C, H, W, k, dptr(ws), stream_ptr()), "dwconv_geo_bwd")
    return gx, gw, gb


@_fake("dwconv_geo_bwd")
def _(gy, x, weight, addend, has_bias):
    C, k = x.shape[1], weight.shape[-1]
    return x.new_empty(gy.shape), x.new_empty(C, 1, k, k), x.new_empty(C if has_bias else 0)


def _dw_grads(ctx, gy, x, w, addend, K):
    """input / weight / bias gradients as the context needs them (one fused call when it needs both kinds);
    ``K``: OPS, or RAW from an eager backward - the kernels' Python functions directly (see ``_eager_front_end``)"""
    need_x = ctx.needs_input_grad[0]
    need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
    gx = gw = gb = None
    gy = _cotangent(gy, need_x and need_w)       # (the fused kernel has the bf16-cotangent instantiation)
    if need_x and need_w:
        gx, gw, gb = K["dwconv_geo_bwd"](gy, x, w, addend, ctx.has_bias)
    elif need_x:
        gx = K["dwconv_geo_dgrad"](gy, w) if addend is None else K["dwconv_geo_dgrad_add"](gy, w, addend)
    elif need_w:
        gw, gb = K["dwconv_geo_wgrad"](gy, x, w.shape[-1], ctx.has_bias)
    if not ctx.has_bias:
        gb = None
    return gx, gw, gb


def _dw_setup(ctx, inputs, output):
    x, w, bias = inputs[:3]
    ctx.save_for_backward(x, w)
    ctx.has_bias = bias is not None


def _dw_backward(ctx, gy):
    x, w = ctx.saved_tensors
    return (*_dw_grads(ctx, gy, x, w, None, OPS), None)


_autograd("dwconv_geo", _dw_setup, _dw_backward)


def dwconv_geo(x, weight, bias=None, out_bf16: bool = False):
    """``out_bf16``: a request (see ``_want_bf16_out``) - the stencil's output as a bf16 tensor for a pointwise consumer"""
    require_hip(x, weight, bias)
    return _dwconv_geo(x, weight, bias, _want_bf16_out(x, out_bf16))


class _DwconvSkip(torch.autograd.Function):
    """``(dwconv_geo(x), x)``: the second output is ``x`` itself for a consumer around the block (the gated blend next
    to the advection's down-projection), so both gradients of ``x`` arrive at this node and the data-gradient kernel
    adds the other one as it stores (``paradis_dwconv_geo_dgrad_add``) - no accumulation pass of the autograd engine
    over the tensor.  Eager only, like ``_ChannelNormSkip``."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_bf16):
        y = _eager_forward("dwconv_geo", (x, weight, bias, out_bf16))
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)
        return y, x

    @staticmethod
    def backward(ctx, gy, gskip):
        x, w = ctx.saved_tensors
        if gy is None:          # only the skip path was used
            return gskip, None, None, None
        return (*_dw_grads(ctx, gy, x, w, gskip, RAW if _plain(gy) else OPS), None)


def dwconv_geo_skip(x, weight, bias=None, out_bf16: bool = False):
    """``(dwconv_geo(x), x)`` for a stencil whose input has another consumer (see ``_DwconvSkip``)."""
    require_hip(x, weight, bias)
    if torch.compiler.is_compiling():
        return _dwconv_geo(x, weight, bias), x
    return _DwconvSkip.apply(x, weight, bias, _want_bf16_out(x, out_bf16))
