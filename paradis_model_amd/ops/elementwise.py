"""elementwise glue: activation, the gated blend (reference model/paradis.py:239-243), adds, the device-scalar scale and
the channel concat / slice copies; csrc/elementwise.hip, csrc/train.hip (scale)"""
from typing import Sequence

import torch
from torch import Tensor

from .._lib import check, dptr, lib, stream_ptr
from ._core import ACT_CODES, _autograd, _define, _f32, _fake, _plane_view, _ws, require_hip
from .gemm import _act_backward, _bias_grads


@_define("activation(Tensor x, int act) -> Tensor")
def _activation(x, act):
    _f32(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib.paradis_act_fwd(dptr(x), dptr(y), x.numel(), act, stream_ptr()), "act_fwd")
    return y


@_fake("activation")
def _(x, act):
    return x.new_empty(x.shape)


def _act_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.act = inputs[1]


def _act_bwd(ctx, gy):
    return _act_backward(gy, ctx.saved_tensors[0], ctx.act), None


_autograd("activation", _act_setup, _act_bwd)


def activation(x, name: str):
    if name not in ("SiLU", "GELU"):
        raise ValueError(f"Unknown activation_fn '{name}'. Allowed: ['SiLU', 'GELU']")
    require_hip(x)
    return _activation(x, ACT_CODES[name])


@_define("gated_blend(Tensor h, Tensor adv, Tensor alpha) -> Tensor")
def _gated_blend(h, adv, alpha):
    _f32(h, adv, alpha)
    h, adv, alpha = h.contiguous(), adv.contiguous(), alpha.contiguous()
    B, C, H, W = h.shape
    out = torch.empty_like(h)
    check(lib.paradis_gated_blend_fwd(dptr(h), dptr(adv), dptr(alpha), dptr(out), B, C, H * W, stream_ptr()),
          "gated_blend_fwd")
    return out


@_fake("gated_blend")
def _(h, adv, alpha):
    return h.new_empty(h.shape)


@_define("gated_blend_backward(Tensor gout, Tensor h, Tensor adv, Tensor alpha) -> (Tensor, Tensor, Tensor)")
def _gated_blend_backward(gout, h, adv, alpha):
    _f32(gout)
    h, adv, alpha, gout = h.contiguous(), adv.contiguous(), alpha.contiguous(), gout.contiguous()
    B, C, H, W = h.shape
    gh, gadv, galpha = torch.empty_like(h), torch.empty_like(h), torch.empty_like(alpha)
    ws = _ws(lib.paradis_gated_blend_bwd_ws_bytes(B, C, H * W), h.device)
    check(lib.paradis_gated_blend_bwd(dptr(gout), dptr(h), dptr(adv), dptr(alpha), dptr(gh), dptr(gadv),
                                      dptr(galpha), B, C, H * W, dptr(ws), stream_ptr()), "gated_blend_bwd")
    return gh, gadv, galpha


@_fake("gated_blend_backward")
def _(gout, h, adv, alpha):
    return h.new_empty(h.shape), h.new_empty(h.shape), alpha.new_empty(alpha.shape)


@_define("gated_blend_backward_out(Tensor gout, Tensor h, Tensor out, Tensor alpha) -> (Tensor, Tensor, Tensor)")
def _gated_blend_backward_out(gout, h, out, alpha):
    """(gh, gadv, galpha) of ``out = h + sigmoid(alpha) (adv - h)`` from the blended output (the gated GEMM epilogue
    never materialises adv): galpha = (1 - sigmoid) sum gout (out - h)."""
    _f32(gout, h, out, alpha)
    gout, h, out = gout.contiguous(), h.contiguous(), out.contiguous()
    B, C, H, W = h.shape
    alpha = alpha.reshape(C).contiguous()
    gh, gadv = torch.empty_like(h), torch.empty_like(h)
    galpha = torch.empty(C, dtype=h.dtype, device=h.device)
    ws = _ws(lib.paradis_gated_blend_bwd_ws_bytes(B, C, H * W), h.device)
    check(lib.paradis_gated_blend_bwd_out(dptr(gout), dptr(h), dptr(out), dptr(alpha), dptr(gh), dptr(gadv),
                                          dptr(galpha), B, C, H * W, dptr(ws), stream_ptr()), "gated_blend_bwd_out")
    return gh, gadv, galpha


@_fake("gated_blend_backward_out")
def _(gout, h, out, alpha):
    return h.new_empty(h.shape), h.new_empty(h.shape), alpha.new_empty(alpha.numel())


def _blend_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _blend_backward(ctx, gout):
    return _gated_blend_backward(gout, *ctx.saved_tensors)


_autograd("gated_blend", _blend_setup, _blend_backward)


def gated_blend(h, adv, alpha):
    """h + sigmoid(alpha)[None,:,None,None] * (adv - h)   (reference model/paradis.py:239-243)"""
    require_hip(h, adv, alpha)
    return _gated_blend(h, adv, alpha)


@_define("add(Tensor a, Tensor b) -> Tensor")
def _add(a, b):
    _f32(a, b)
    assert a.shape == b.shape
    a, b = a.contiguous(), b.contiguous()
    y = torch.empty_like(a)
    check(lib.paradis_add(dptr(a), dptr(b), dptr(y), a.numel(), stream_ptr()), "add")
    return y


@_fake("add")
def _(a, b):
    return a.new_empty(a.shape)


_autograd("add", lambda ctx, inputs, output: None, lambda ctx, gy: (gy, gy))


def add(a, b):
    require_hip(a, b)
    return _add(a, b)


@_define("add_bias_map(Tensor x, Tensor bmap) -> Tensor")
def _add_bias_map(x, bmap):
    _f32(x, bmap)
    x, bmap = x.contiguous(), bmap.contiguous()
    assert x.shape[1:] == bmap.shape
    y = torch.empty_like(x)
    check(lib.paradis_add_bcast(dptr(x), dptr(bmap), dptr(y), bmap.numel(), x.shape[0], stream_ptr()), "add_bcast")
    return y


@_fake("add_bias_map")
def _(x, bmap):
    return x.new_empty(x.shape)


def _abm_backward(ctx, gy):
    gmap = None
    if ctx.needs_input_grad[1]:
        gmap = _bias_grads(gy, False, True)[1]
    return gy, gmap


_autograd("add_bias_map", lambda ctx, inputs, output: None, _abm_backward)


def add_bias_map(x, bmap):
    """x[B,C,H,W] + bmap[C,H,W] (standalone GlobalBias, reference model/blocks.py:196)"""
    require_hip(x, bmap)
    return _add_bias_map(x, bmap)


@_define("scale(Tensor x, Tensor s) -> Tensor")
def _scale(x, s):
    """x * s for a one-element device tensor s (no host sync)"""
    _f32(x, s)
    x, s = x.contiguous(), s.contiguous()
    out = torch.empty_like(x)
    check(lib.paradis_scale(dptr(x), dptr(s), dptr(out), x.numel(), stream_ptr()), "scale")
    return out


@_fake("scale")
def _(x, s):
    return x.new_empty(x.shape)


@_define("concat_channels(Tensor[] parts) -> Tensor", autocast=False)
def _concat_channels(parts):
    """cat(parts, dim=1) for [B,C_i,H,W] tensors (channel slices accepted) by strided block copies."""
    _f32(*parts)
    B = parts[0].shape[0]
    H, W = parts[0].shape[-2:]
    chans = [p.shape[1] for p in parts]
    P, Ct = H * W, sum(chans)
    out = torch.empty(B, Ct, H, W, dtype=parts[0].dtype, device=parts[0].device)
    off = 0
    for p, c in zip(parts, chans):
        p, bs = _plane_view(p)
        check(lib.paradis_copy_channels(dptr(p), bs, dptr(out[:, off:]), Ct * P, B, c * P, stream_ptr()),
              "copy_channels")
        off += c
    return out


@_fake("concat_channels")
def _(parts):
    B, _, H, W = parts[0].shape
    return parts[0].new_empty(B, sum(p.shape[1] for p in parts), H, W)


@_define("slice_channels(Tensor x, int off, int c) -> Tensor")
def _slice_channels(x, off, c):
    """contiguous copy of x[:, off:off+c]"""
    _f32(x)
    x = x.contiguous()
    B, Ct, H, W = x.shape
    P = H * W
    g = torch.empty(B, c, H, W, dtype=x.dtype, device=x.device)
    check(lib.paradis_copy_channels(dptr(x[:, off:]), Ct * P, dptr(g), c * P, B, c * P, stream_ptr()),
          "copy_channels")
    return g


@_fake("slice_channels")
def _(x, off, c):
    return x.new_empty(x.shape[0], c, x.shape[2], x.shape[3])


def _cat_setup(ctx, inputs, output):
    ctx.chans = [p.shape[1] for p in inputs[0]]


def _cat_backward(ctx, gout):
    grads, off = [], 0
    need = ctx.needs_input_grad[0]
    for i, c in enumerate(ctx.chans):
        grads.append(_slice_channels(gout, off, c) if need[i] else None)
        off += c
    return (grads,)


_autograd("concat_channels", _cat_setup, _cat_backward)


def concat_channels(parts: Sequence[Tensor]):
    require_hip(*parts)
    return _concat_channels(list(parts))
