"""a11 / a14 resampling: coarsening average and longitude-periodic upsampling; csrc/resample.hip"""
import torch
from torch import Tensor

from .._lib import check, dptr, lib, stream_ptr
from ._core import _autograd, _define, _f32, _fake, _planes_hw, require_hip
from .stencil import _dwconv_geo


@_define("avgpool_geo(Tensor x, int stride) -> Tensor")
def _avgpool_geo(x, stride):
    _f32(x)
    x = x.contiguous()
    planes, H, W = _planes_hw(x)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(*x.shape[:-2], Ho, Wo, dtype=x.dtype, device=x.device)
    check(lib.paradis_avgpool_geo_fwd(dptr(x), dptr(y), planes, H, W, stride, stream_ptr()), "avgpool_geo_fwd")
    return y


@_fake("avgpool_geo")
def _(x, stride):
    H, W = x.shape[-2:]
    return x.new_empty(*x.shape[:-2], (H - 1) // stride + 1, (W - 1) // stride + 1)


@_define("avgpool_geo_backward(Tensor gy, int H, int W, int stride) -> Tensor")
def _avgpool_geo_backward(gy, H, W, stride):
    _f32(gy)
    gy = gy.contiguous()
    gx = torch.empty(*gy.shape[:-2], H, W, dtype=gy.dtype, device=gy.device)
    check(lib.paradis_avgpool_geo_bwd(dptr(gy), dptr(gx), gx.numel() // (H * W), H, W, stride, stream_ptr()),
          "avgpool_geo_bwd")
    return gx


@_fake("avgpool_geo_backward")
def _(gy, H, W, stride):
    return gy.new_empty(*gy.shape[:-2], H, W)


def _pool_setup(ctx, inputs, output):
    ctx.meta = (inputs[0].shape[-2], inputs[0].shape[-1], inputs[1])


def _pool_backward(ctx, gy):
    return _avgpool_geo_backward(gy, *ctx.meta), None


_autograd("avgpool_geo", _pool_setup, _pool_backward)

_BOX_WEIGHTS = {}


def avgpool_geo(x, stride: int):
    if stride < 1:
        raise ValueError("Coarsening factor must be >=1")
    require_hip(x)
    if stride == 1:
        # stride 1 = depthwise 5x5 stencil with uniform taps 1/25: reuse the LDS-tiled kernels
        # (forward 2.8x, backward 5x faster than the generic strided kernels)
        key = (x.shape[1], str(x.device))
        w = _BOX_WEIGHTS.get(key)
        if w is None:
            w = torch.full((x.shape[1], 1, 5, 5), 1.0 / 25.0, dtype=torch.float32, device=x.device)
            # only a tensor made by an eager call is cached: one made while tracing (FakeTensorMode, torch.compile) can
            # be a fake without storage, and a later eager call would hand the kernel its null pointer
            if type(w) is Tensor and not torch.compiler.is_compiling():
                _BOX_WEIGHTS[key] = w
        return _dwconv_geo(x, w, None)
    return _avgpool_geo(x, int(stride))


@_define("upsample_lonp(Tensor x, int nlat, int nlon) -> Tensor")
def _upsample_lonp(x, nlat, nlon):
    _f32(x)
    x = x.contiguous()
    planes, Hc, Wc = _planes_hw(x)
    y = torch.empty(*x.shape[:-2], nlat, nlon, dtype=x.dtype, device=x.device)
    check(lib.paradis_upsample_lonp_fwd(dptr(x), dptr(y), planes, Hc, Wc, nlat, nlon, stream_ptr()),
          "upsample_lonp_fwd")
    return y


@_fake("upsample_lonp")
def _(x, nlat, nlon):
    return x.new_empty(*x.shape[:-2], nlat, nlon)


@_define("upsample_lonp_backward(Tensor gy, int Hc, int Wc) -> Tensor")
def _upsample_lonp_backward(gy, Hc, Wc):
    _f32(gy)
    gy = gy.contiguous()
    nlat, nlon = gy.shape[-2:]
    gx = torch.empty(*gy.shape[:-2], Hc, Wc, dtype=gy.dtype, device=gy.device)
    check(lib.paradis_upsample_lonp_bwd(dptr(gy), dptr(gx), gx.numel() // (Hc * Wc), Hc, Wc, nlat, nlon,
                                        stream_ptr()), "upsample_lonp_bwd")
    return gx


@_fake("upsample_lonp_backward")
def _(gy, Hc, Wc):
    return gy.new_empty(*gy.shape[:-2], Hc, Wc)


def _up_setup(ctx, inputs, output):
    ctx.meta = tuple(inputs[0].shape[-2:])


def _up_backward(ctx, gy):
    return _upsample_lonp_backward(gy, *ctx.meta), None, None


_autograd("upsample_lonp", _up_setup, _up_backward)


def upsample_lonp(x, nlat: int, nlon: int):
    if tuple(x.shape[-2:]) == (int(nlat), int(nlon)):
        return x   # equal sizes: ATen's align_corners interpolation is the exact identity
    require_hip(x)
    return _upsample_lonp(x, int(nlat), int(nlon))
