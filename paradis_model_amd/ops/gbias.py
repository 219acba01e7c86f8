"""a9 GlobalBias map (reference model/blocks.py:188-196): the low-rank map, its un-projected form for the GEMM epilogue
and the adjoint of that projection; csrc/gbias.hip"""
import torch

from .._lib import check, dptr, lib, stream_ptr
from ._core import _autograd, _define, _f32, _fake, _ws, require_hip


@_define("global_bias_map(Tensor A, Tensor U, Tensor V, Tensor? Pw) -> (Tensor, Tensor)")
def _global_bias_map(A, U, V, Pw):
    _f32(A, U, V, Pw)
    A, U, V = A.contiguous(), U.contiguous(), V.contiguous()
    Cin, R = A.shape
    H, W = U.shape[1], V.shape[1]
    if Pw is not None:
        Pw = Pw.contiguous()
        Co = Pw.shape[0]
        m8 = torch.empty(Cin, H, W, dtype=A.dtype, device=A.device)
    else:
        Co, m8 = Cin, A.new_empty(0)
    out = torch.empty(Co, H, W, dtype=A.dtype, device=A.device)
    check(lib.paradis_global_bias_map_fwd(dptr(A), dptr(U), dptr(V), dptr(Pw), dptr(m8) if Pw is not None else None,
                                          dptr(out), Cin, Co, R, H, W, stream_ptr()), "global_bias_map_fwd")
    return out, m8


@_fake("global_bias_map")
def _(A, U, V, Pw):
    Cin, H, W = A.shape[0], U.shape[1], V.shape[1]
    if Pw is not None:
        return A.new_empty(Pw.shape[0], H, W), A.new_empty(Cin, H, W)
    return A.new_empty(Cin, H, W), A.new_empty(0)


@_define("global_bias_map_backward(Tensor gmap, Tensor A, Tensor U, Tensor V, Tensor? Pw, Tensor m8) "
         "-> (Tensor, Tensor, Tensor, Tensor)")
def _global_bias_map_backward(gmap, A, U, V, Pw, m8):
    _f32(gmap)
    A, U, V = A.contiguous(), U.contiguous(), V.contiguous()
    Cin, R = A.shape
    H, W = U.shape[1], V.shape[1]
    gmap = gmap.contiguous()
    Co = gmap.shape[0]
    has_proj = Pw is not None
    gA, gU, gV = torch.empty_like(A), torch.empty_like(U), torch.empty_like(V)
    gPw = torch.empty_like(Pw) if has_proj else A.new_empty(0)
    ws = _ws(lib.paradis_global_bias_map_bwd_ws_bytes(Cin, Co, R, H, W), A.device)
    check(lib.paradis_global_bias_map_bwd(dptr(gmap), dptr(A), dptr(U), dptr(V),
                                          dptr(Pw.contiguous()) if has_proj else None,
                                          dptr(m8) if has_proj else None, dptr(gA), dptr(gU), dptr(gV),
                                          dptr(gPw) if has_proj else None, Cin, Co, R, H, W, dptr(ws),
                                          stream_ptr()), "global_bias_map_bwd")
    return gA, gU, gV, gPw


@_fake("global_bias_map_backward")
def _(gmap, A, U, V, Pw, m8):
    return (A.new_empty(A.shape), U.new_empty(U.shape), V.new_empty(V.shape),
            A.new_empty(Pw.shape) if Pw is not None else A.new_empty(0))


def _gbm_setup(ctx, inputs, output):
    A, U, V, Pw = inputs
    ctx.save_for_backward(A, U, V, Pw, output[1])
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)


def _gbm_backward(ctx, gmap, gm8=None):
    A, U, V, Pw, m8 = ctx.saved_tensors
    if gmap is None:
        return None, None, None, None
    gA, gU, gV, gPw = _global_bias_map_backward(gmap, A, U, V, Pw, m8)
    return gA, gU, gV, (gPw if Pw is not None else None)


_autograd("global_bias_map", _gbm_setup, _gbm_backward)


def global_bias_map(A, U, V, Pw=None):
    require_hip(A, U, V, Pw)
    return _global_bias_map(A, U, V, Pw)[0]


@_define("global_bias_m8(Tensor A, Tensor U, Tensor V) -> Tensor")
def _global_bias_m8(A, U, V):
    """Un-projected rank-R map m8[Cin,H,W]; the projection to the layer width is applied inside
    the GEMM epilogue (``pointwise(..., bias_proj=(m8, Pw))``) so the [Co,H,W] map is never stored."""
    _f32(A, U, V)
    A, U, V = A.contiguous(), U.contiguous(), V.contiguous()
    Cin, R = A.shape
    H, W = U.shape[1], V.shape[1]
    m8 = torch.empty(Cin, H, W, dtype=A.dtype, device=A.device)
    check(lib.paradis_global_bias_m8_fwd(dptr(A), dptr(U), dptr(V), dptr(m8), Cin, R, H, W, stream_ptr()),
          "global_bias_m8_fwd")
    return m8


@_fake("global_bias_m8")
def _(A, U, V):
    return A.new_empty(A.shape[0], U.shape[1], V.shape[1])


@_define("global_bias_m8_backward(Tensor gm8, Tensor A, Tensor U, Tensor V) -> (Tensor, Tensor, Tensor)")
def _global_bias_m8_backward(gm8, A, U, V):
    _f32(gm8)
    A, U, V = A.contiguous(), U.contiguous(), V.contiguous()
    Cin, R = A.shape
    H, W = U.shape[1], V.shape[1]
    gm8 = gm8.contiguous()
    gA, gU, gV = torch.empty_like(A), torch.empty_like(U), torch.empty_like(V)
    ws = _ws(lib.paradis_global_bias_map_bwd_ws_bytes(Cin, Cin, R, H, W), A.device)
    check(lib.paradis_global_bias_m8_bwd(dptr(gm8), dptr(A), dptr(U), dptr(V), dptr(gA), dptr(gU), dptr(gV),
                                         Cin, R, H, W, dptr(ws), stream_ptr()), "global_bias_m8_bwd")
    return gA, gU, gV


@_fake("global_bias_m8_backward")
def _(gm8, A, U, V):
    return A.new_empty(A.shape), U.new_empty(U.shape), V.new_empty(V.shape)


def _gb8_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _gb8_backward(ctx, gm8):
    return _global_bias_m8_backward(gm8, *ctx.saved_tensors)


_autograd("global_bias_m8", _gb8_setup, _gb8_backward)


def global_bias_m8(A, U, V):
    require_hip(A, U, V)
    return _global_bias_m8(A, U, V)


@_define("global_bias_proj_backward(Tensor gmap, Tensor m8, Tensor pw) -> (Tensor, Tensor)")
def _global_bias_proj_backward(gmap, m8, pw):
    """adjoint of the projection fused into the GEMM epilogue: gmap[Co,H,W] -> (gPw[Co,cin], gm8[cin,H,W])"""
    _f32(gmap, m8, pw)
    gmap, m8, pw = gmap.contiguous(), m8.contiguous(), pw.contiguous()
    Co, cin = pw.shape
    gpw, gm8 = torch.empty_like(pw), torch.empty_like(m8)
    check(lib.paradis_global_bias_proj_bwd(dptr(gmap), dptr(m8), dptr(pw), dptr(gpw), dptr(gm8), cin, Co,
                                           m8.shape[1] * m8.shape[2], stream_ptr()), "global_bias_proj_bwd")
    return gpw, gm8


@_fake("global_bias_proj_backward")
def _(gmap, m8, pw):
    return pw.new_empty(pw.shape), m8.new_empty(m8.shape)
