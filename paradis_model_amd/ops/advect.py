"""a3-a5 semi-Lagrangian advection core (reference model/advection.py:129-169); csrc/advect*.hip"""
from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from .. import ops      # settings (ops.ADVECT_FLAGS) are read from the package at call time
from .._lib import dptr, lib, stream_ptr
from ._core import (MODE_CODES, _autograd, _define, _eager_front_end, _f32, _fake, _plane_view, _ws, require_hip)


class AdvectGeometry:
    """Device tables + scalars derived from the lat/lon grids once per module
    (the reference's non-persistent buffers, model/advection.py:58-72)."""

    def __init__(self, lat_grid: Tensor, lon_grid: Tensor):
        lat = lat_grid.detach().to(torch.float32).cpu().contiguous()
        lon = lon_grid.detach().to(torch.float32).cpu().contiguous()
        self.H, self.W = lat.shape
        # tables are evaluated once on the host in fp32, as the reference's CPU path would
        self.sin_lat = torch.sin(lat).contiguous()
        self.cos_lat = torch.cos(lat).contiguous()
        self.lon = lon
        self.min_lat = float(lat.min())
        self.min_lon = float(lon.min())
        self.d_lat = float(lat.max() - lat.min())
        self.d_lon = float(lon.max() - lon.min())
        # regular lat-lon grid: latitude depends on the row only, longitude on the column only
        self.separable = bool((lat == lat[:, :1]).all()) and bool((lon == lon[:1, :]).all())
        # arrival latitude in cells, (lat - min_lat) (H-1)/d_lat, in double; the padding p is added per mode
        cells = (lat.double() - self.min_lat) * ((self.H - 1.0) / self.d_lat) if self.d_lat > 0 else lat.double() * 0
        self.lat_cells = {p: (cells + float(p)).to(torch.float32).contiguous() for p in (1, 2)}
        self._dev = {}

    def tables(self, device, p: int = 2):
        """(sin_lat, cos_lat, lat_cells, lon) on ``device``; lat_cells = p + (lat - min_lat)(H-1)/d_lat as fp32"""
        key = (str(device), p)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.sin_lat, self.cos_lat, self.lat_cells[p], self.lon))
        return self._dev[key]


_ADV_TABLES = "Tensor sin_lat, Tensor cos_lat, Tensor lat_cells, Tensor lon"
_ADV_GEOM = "float dt, float min_lat, float min_lon, float d_lat, float d_lon, int mode, int flags"


# One forward and one backward launch serve both ops: ``u`` / ``v`` are [B,K,H,W] planes whose batches lie ``uv_bs``
# elements apart - two tensors, or the two halves of one [B,2K,H,W] velocity tensor; ``tables`` / ``geom`` are the
# schema's ``_ADV_TABLES`` / ``_ADV_GEOM`` arguments (``geom[-1]`` = flags).
def _launch_fwd(field, u, v, uv_bs, tables, geom):
    B, K, H, W = field.shape
    field, f_bs = _plane_view(field)
    out = torch.empty(B, K, H, W, dtype=field.dtype, device=field.device)
    ws = _ws(lib.paradis_sl_advect_ws_bytes(B, K, H, W, geom[-1]), field.device)
    _lib.call("sl_advect_fwd", 16.0 * B * K * H * W,   # algorithmic bytes: 16 B / gather point
              dptr(field), dptr(u), dptr(v), dptr(out), *map(dptr, tables), B, K, H, W,
              f_bs, uv_bs, K * H * W, *geom, dptr(ws), stream_ptr())
    return out


def _launch_bwd(gout, field, u, v, uv_bs, gu, gv, guv_bs, tables, geom):
    """writes the velocity gradients into ``gu`` / ``gv`` (batches ``guv_bs`` apart) and returns the field's"""
    B, K, H, W = gout.shape
    P = K * H * W
    gout = gout.contiguous()
    field, f_bs = _plane_view(field)
    gfield = torch.empty(B, K, H, W, dtype=gout.dtype, device=gout.device)
    ws = _ws(lib.paradis_sl_advect_ws_bytes(B, K, H, W, geom[-1]), gout.device)
    _lib.call("sl_advect_bwd", 28.0 * B * K * H * W,   # algorithmic bytes: 28 B / gather point
              dptr(gout), dptr(field), dptr(u), dptr(v), dptr(gfield), dptr(gu), dptr(gv), *map(dptr, tables),
              B, K, H, W, P, f_bs, uv_bs, P, guv_bs, *geom, dptr(ws), stream_ptr())
    return gfield


def _uv_views(u: Tensor, v: Tensor):
    """(u, v, their common batch stride): in place where both are plane views the same distance apart"""
    u, u_bs = _plane_view(u)
    v, v_bs = _plane_view(v)
    if u_bs != v_bs:
        u, v = u.contiguous(), v.contiguous()
        u_bs = u.shape[1] * u.shape[2] * u.shape[3]
    return u, v, u_bs


@_define(f"sl_advect(Tensor field, Tensor u, Tensor v, {_ADV_TABLES}, {_ADV_GEOM}) -> Tensor")
def _sl_advect(field, u, v, sl, cl, lc, lo, *geom):
    _f32(field, u, v)
    return _launch_fwd(field, *_uv_views(u, v), (sl, cl, lc, lo), geom)


@_fake("sl_advect")
def _(field, u, v, sl, cl, lc, lo, dt, min_lat, min_lon, d_lat, d_lon, mode, flags):
    return field.new_empty(field.shape)


@_define(f"sl_advect_backward(Tensor gout, Tensor field, Tensor u, Tensor v, {_ADV_TABLES}, "
         f"{_ADV_GEOM}) -> (Tensor, Tensor, Tensor)")
def _sl_advect_backward(gout, field, u, v, sl, cl, lc, lo, *geom):
    _f32(gout, field, u, v)
    gu = torch.empty(gout.shape, dtype=gout.dtype, device=gout.device)
    gv = torch.empty_like(gu)
    _, K, H, W = gout.shape
    gfield = _launch_bwd(gout, field, *_uv_views(u, v), gu, gv, K * H * W, (sl, cl, lc, lo), geom)
    return gfield, gu, gv


@_fake("sl_advect_backward")
def _(gout, field, u, v, sl, cl, lc, lo, dt, min_lat, min_lon, d_lat, d_lon, mode, flags):
    return gout.new_empty(gout.shape), gout.new_empty(gout.shape), gout.new_empty(gout.shape)


def _adv_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:7])
    ctx.geom = inputs[7:]


def _adv_backward(ctx, gout):
    gf, gu, gv = _sl_advect_backward(gout, *ctx.saved_tensors, *ctx.geom)
    return (gf, gu, gv) + (None,) * 11


_autograd("sl_advect", _adv_setup, _adv_backward)


@_define(f"sl_advect_vel(Tensor field, Tensor vel, {_ADV_TABLES}, {_ADV_GEOM}) -> Tensor")
def _sl_advect_vel(field, vel, sl, cl, lc, lo, *geom):
    """Same operator taking the velocity tensor [B,2K,H,W] whole (channels [0,K) = u, [K,2K) = v,
    reference model/paradis.py:236-237): no slice views, and the velocity gradient is written in
    place into one [B,2K,H,W] tensor."""
    _f32(field, vel)
    _, K, H, W = field.shape
    vel = vel.contiguous()
    return _launch_fwd(field, vel[:, :K], vel[:, K:], 2 * K * H * W, (sl, cl, lc, lo), geom)


@_fake("sl_advect_vel")
def _(field, vel, sl, cl, lc, lo, dt, min_lat, min_lon, d_lat, d_lon, mode, flags):
    return field.new_empty(field.shape)


@_define(f"sl_advect_vel_backward(Tensor gout, Tensor field, Tensor vel, {_ADV_TABLES}, "
         f"{_ADV_GEOM}) -> (Tensor, Tensor)")
def _sl_advect_vel_backward(gout, field, vel, sl, cl, lc, lo, *geom):
    _f32(gout, field, vel)
    _, K, H, W = gout.shape
    P2 = 2 * K * H * W
    vel = vel.contiguous()
    gvel = torch.empty_like(vel)
    gfield = _launch_bwd(gout, field, vel[:, :K], vel[:, K:], P2, gvel[:, :K], gvel[:, K:], P2, (sl, cl, lc, lo), geom)
    return gfield, gvel


@_fake("sl_advect_vel_backward")
def _(gout, field, vel, sl, cl, lc, lo, dt, min_lat, min_lon, d_lat, d_lon, mode, flags):
    return gout.new_empty(gout.shape), vel.new_empty(vel.shape)


def _advv_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:6])
    ctx.geom = inputs[6:]


def _advv_backward(ctx, saved, K, gout):
    gf, gvel = K["sl_advect_vel_backward"](gout, *saved, *ctx.geom)
    return (gf, gvel) + (None,) * 11


# (registers the formula and returns it as a plain autograd.Function for eager recording calls: ``_core``)
_AdvectVelEager = _eager_front_end("sl_advect_vel", _advv_setup, _advv_backward, widen=True)


ADVECT_GENERIC, ADVECT_TILED, ADVECT_SEPARABLE, ADVECT_TILES, ADVECT_STRIPS = 1, 2, 4, 8, 16     # include/paradis_hip.h PARADIS_ADVECT_*


def advect_flags(tiled: bool = False, halo: Optional[int] = None, halo_bwd: Optional[int] = None,
                 generic: bool = False, tiles: bool = False, strips: bool = False) -> int:
    """``flags`` of the advection ops: force the windowed schedule and/or its longitude halo (padded cells;
    ``halo_bwd`` overrides it for the backward kernel), the generic whole-plane kernel, or (``tiles``, diagnostic)
    the tile schedule of rounds 2-3 in place of the strips; ``strips``: the backward's 128-column strips where the
    full-circle ring (W <= 256) would run."""
    return ((ADVECT_TILED if tiled else 0) | (ADVECT_GENERIC if generic else 0) | (ADVECT_TILES if tiles else 0)
            | (ADVECT_STRIPS if strips else 0)
            | (((int(halo) + 1) << 8) if halo is not None else 0)
            | (((int(halo_bwd) + 1) << 16) if halo_bwd is not None else 0))


def _geom_args(geom: AdvectGeometry, device, dt: float, mode: str, flags: Optional[int]):
    if mode not in MODE_CODES:
        raise ValueError(f"interpolation must be one of {list(MODE_CODES)}")
    sl, cl, lc, lo = geom.tables(device, 2 if mode == "bicubic" else 1)
    flags = ops.ADVECT_FLAGS if flags is None else int(flags)
    if geom.separable:
        flags |= ADVECT_SEPARABLE
    return sl, cl, lc, lo, float(dt), geom.min_lat, geom.min_lon, geom.d_lat, geom.d_lon, MODE_CODES[mode], flags


def sl_advect_vel(field, vel, geom: AdvectGeometry, dt: float, mode: str = "bicubic", flags: Optional[int] = None):
    require_hip(field, vel)
    B, K, H, W = field.shape
    assert vel.shape == (B, 2 * K, H, W) and (H, W) == (geom.H, geom.W)
    args = (field, vel, *_geom_args(geom, field.device, dt, mode, flags))
    if torch.is_grad_enabled() and not torch.compiler.is_compiling():
        return _AdvectVelEager.apply(*args)
    return _sl_advect_vel(*args)


def sl_advect(field, u, v, geom: AdvectGeometry, dt: float, mode: str = "bicubic", flags: Optional[int] = None):
    """[B,K,H,W] x3 -> [B,K,H,W]; fused pole-mean / departure / gather / pole-mean."""
    require_hip(field, u, v)
    assert tuple(field.shape[-2:]) == (geom.H, geom.W) and u.shape == field.shape and v.shape == field.shape
    return _sl_advect(field, u, v, *_geom_args(geom, field.device, dt, mode, flags))
