"""a6 pointwise channel mixing on the matrix cores with fused epilogue
    y = residual + act(W x + bias + bias_map)
(reference model/blocks.py:86,110 + :196 + activation + the residual adds of paradis.py:246,253), its gradient GEMMs, the
bias / activation gradients and the weight-gradient side stream; csrc/gemm*.hip.  The arithmetic schemes are described
where they are selected (``ops/__init__.py``), the weight images in ``_images.py``."""
from typing import Optional

import torch

from .. import _lib
from .. import ops      # settings (ops.GEMM_SCHEME, ops.BF16_STORAGE) are read from the package at call time
from .._lib import check, dptr, lib, stream_ptr
from ._core import (ACT_CODES, AMAX_PARTIALS, GEMM_BF16, GEMM_EXACT, GEMM_F16X2, IO_DY16, IO_X16, IO_Y16, IO_Z16, RAW,
                    _define, _eager_front_end, _f32, _f32_or_bf16, _fake, _is16, _plane_view, _stores_bf16, _ws,
                    autocast_scheme, require_hip)
from ._images import _split_image, _stash_wt, _take_wt


@_define("amax_partials(Tensor x) -> Tensor")
def _amax_partials(x):
    """int32[AMAX_PARTIALS]: bit patterns of partial maxima of |x| ([B,C,H,W], channel-sliced views allowed);
    the opt-in f16x2 GEMMs take the maximum of the words as the tensor's largest magnitude.  One read pass."""
    _f32(x)
    x, x_bs = _plane_view(x)
    B, C, H, W = x.shape
    out = torch.empty(AMAX_PARTIALS, dtype=torch.int32, device=x.device)
    check(lib.paradis_amax_partials(dptr(x), B, C * H * W, x_bs, dptr(out), stream_ptr()), "amax_partials")
    return out


@_fake("amax_partials")
def _(x):
    return x.new_empty(AMAX_PARTIALS, dtype=torch.int32)


@_define("pointwise(Tensor x, Tensor weight, Tensor? bias, Tensor? bmap, Tensor? residual, int act, "
         "Tensor? x_pre, int x_act, bool defer_act_grad, Tensor? m8, Tensor? pw, bool save_z, int scheme, "
         "Tensor? gate, bool want_wt_image=False, bool out_bf16=False) -> (Tensor, Tensor, Tensor)", autocast=((0, 6), 12))
def _pointwise(x, weight, bias, bmap, residual, act, x_pre, x_act, defer_act_grad, m8, pw, save_z, scheme, gate,
               want_wt_image=False, out_bf16=False):
    """y = residual + act(W x + bias + bias_map); second output = pre-activation z (empty unless save_z);
    third = amax partials of x (f16x2 scheme; empty otherwise), kept for the weight gradient.
    ``scheme``: GEMM arithmetic (GEMM_EXACT / GEMM_BF16X3 / GEMM_F16X2); the backward uses the same.
    ``gate`` [Co] (with ``residual``): y = residual + sigmoid(gate)[:,None] * (act(...) - residual) - the gated blend
    of reference model/paradis.py:239-243 in the GEMM epilogue (``ops.gated_blend`` without the advected tensor).
    ``want_wt_image``: a hint, no effect on the result - the backward of this call will need the split image of W^T
    (x requires a gradient): both images are then written by one launch and cached.

    Activation-gradient hand-off between two chained ops (GMBlock drives it):
      * ``defer_act_grad`` (producer): the op's backward receives d(pre-activation) directly and
        skips its own act' pass; the consumer reads the returned ``z``.
      * ``x_pre`` / ``x_act`` (consumer): x = act(x_pre) was produced by such an op; the consumer's
        dgrad multiplies by act'(x_pre) in the GEMM epilogue, so what it returns as the gradient of
        ``x`` already is the producer's d(pre-activation).
    """
    _f32(weight, bias, bmap, residual, m8, pw, gate)
    _f32_or_bf16(scheme, x)
    x, x_bs = _plane_view(x)
    B, Ci, H, W = x.shape
    Co = weight.shape[0]
    P = H * W
    assert weight.numel() == Co * Ci, "weight/in-channel mismatch"
    x16 = _is16(x)
    if x16 or out_bf16:
        # bf16-STORED activations (bf16-mixed scheme only; the public wrapper decides): ``out_bf16`` writes y and z as
        # bf16 tensors - what autocast's conv2d returns in the reference (model/blocks.py:86,110)
        if scheme != GEMM_BF16 or (out_bf16 and residual is not None):
            raise RuntimeError("bf16-stored tensors need the bf16-mixed GEMM scheme (and a bf16 output no residual)")
        if x16 and (P % 8 or x_bs % 8 or x.data_ptr() % 16):
            raise RuntimeError("a bf16-stored GEMM input needs H W % 8 == 0 and 16-byte aligned planes")
    if gate is not None:
        assert residual is not None and gate.numel() == Co, "a gate needs the residual it blends with, one value per channel"
        gate = gate.reshape(Co).contiguous()
    res_bs = 0
    if residual is not None:
        residual, res_bs = _plane_view(residual)
    if bmap is not None:
        bmap = bmap.contiguous()
    y = torch.empty(B, Co, H, W, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    cin, pwt = 0, None
    if pw is not None:
        m8, pw = m8.contiguous(), pw.contiguous()
        cin = pw.shape[1]
        assert pw.shape[0] == Co and m8.shape == (cin, H, W) and bmap is None
        assert Co % 4 == 0 and cin <= 16, "fused GlobalBias projection needs Co % 4 == 0 and <= 16 bias channels"
        pwt = pw.t().contiguous()   # [cin, Co]: four consecutive output rows per 16-byte load
    z = torch.empty_like(y) if (save_z and act != 0) else y.new_empty(0)
    w2 = weight.reshape(Co, Ci).contiguous()
    w2t = wsp = None
    x_amax = x.new_empty(0, dtype=torch.int32)
    _stash_wt(weight, None)
    if scheme != GEMM_EXACT:
        wsp, wtsp_out = _split_image(weight, Co, Ci, False, scheme, bool(want_wt_image))   # split planes in tile order
        _stash_wt(weight, wtsp_out)
        if scheme == GEMM_F16X2:
            x_amax = torch.empty(AMAX_PARTIALS, dtype=torch.int32, device=x.device)
            check(lib.paradis_amax_partials(dptr(x), B, Ci * P, x_bs, dptr(x_amax), stream_ptr()), "amax_partials")
    elif Ci % 16 == 0 and Co % 4 == 0 and Co * Ci >= 4096:
        # [Ci,Co] copy of the weights: makes the A operand row-contiguous for the LDS-DMA kernel
        w2t = torch.empty(Ci, Co, dtype=torch.float32, device=x.device)
        check(lib.paradis_transpose(dptr(w2), dptr(w2t), Co, Ci, stream_ptr()), "transpose")
    head = (dptr(w2), dptr(w2t), dptr(wsp), scheme, dptr(x_amax) if x_amax.numel() else None, dptr(x), dptr(bias),
            dptr(bmap), dptr(m8) if cin else None, dptr(pwt) if cin else None, cin, dptr(residual))
    tail = (dptr(y), dptr(z) if z.numel() else None, B, Co, Ci, P, x_bs, res_bs, Co * P, act, stream_ptr())
    if x16 or out_bf16:
        _lib.call("pw_gemm_fwd", 2.0 * B * Co * Ci * P, dptr(wsp), dptr(x), dptr(bias), dptr(bmap),
                  dptr(m8) if cin else None, dptr(pwt) if cin else None, cin, dptr(residual), dptr(gate), dptr(y),
                  dptr(z) if z.numel() else None, B, Co, Ci, P, x_bs, res_bs, Co * P, act,
                  (IO_X16 if x16 else 0) | (IO_Y16 if out_bf16 else 0), stream_ptr(), symbol="pw_gemm_fwd16")
        return y, z, x_amax
    if gate is None:
        _lib.call("pw_gemm_fwd", 2.0 * B * Co * Ci * P, *head, *tail)
    else:
        _lib.call("pw_gemm_fwd", 2.0 * B * Co * Ci * P, *head, dptr(gate), *tail, symbol="pw_gemm_fwd_gated")
    return y, z, x_amax


@_fake("pointwise")
def _(x, weight, bias, bmap, residual, act, x_pre, x_act, defer_act_grad, m8, pw, save_z, scheme, gate,
      want_wt_image=False, out_bf16=False):
    B, _, H, W = x.shape
    y = x.new_empty(B, weight.shape[0], H, W, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    return (y, (y.new_empty(y.shape) if (save_z and act != 0) else y.new_empty(0)),
            x.new_empty(AMAX_PARTIALS if scheme == GEMM_F16X2 else 0, dtype=torch.int32))


@_define("act_backward(Tensor gy, Tensor z, int act, bool out_bf16=False) -> Tensor")
def _act_backward(gy, z, act, out_bf16=False):
    """``out_bf16`` (bf16-mixed scheme): d(pre-activation) as a bf16 tensor - the operand both gradient GEMMs of the layer
    would round to bf16 on load (same values; the reference's autocast backward holds this tensor in bf16 as well)"""
    _f32(gy, z)
    gy, z = gy.contiguous(), z.contiguous()
    if out_bf16 and gy.numel() % 4 == 0:
        dz = torch.empty(gy.shape, dtype=torch.bfloat16, device=gy.device)
        check(lib.paradis_act_bwd16(dptr(gy), dptr(z), dptr(dz), gy.numel(), act, stream_ptr()), "act_bwd16")
        return dz
    dz = torch.empty_like(gy)
    check(lib.paradis_act_bwd(dptr(gy), dptr(z), dptr(dz), gy.numel(), act, stream_ptr()), "act_bwd")
    return dz


@_fake("act_backward")
def _(gy, z, act, out_bf16=False):
    return gy.new_empty(gy.shape, dtype=torch.bfloat16 if (out_bf16 and gy.numel() % 4 == 0) else gy.dtype)


@_define("pw_gemm_dgrad(Tensor dz, Tensor weight, Tensor? zmul, int x_act, Tensor? dz_amax, int scheme, "
         "Tensor? wt_image=None, bool out_bf16=False) -> Tensor", autocast=((0, 2), 5))
def _pw_gemm_dgrad(dz, weight, zmul, x_act, dz_amax, scheme, wt_image=None, out_bf16=False):
    """gx = W^T dz (* act'(zmul) when the producing layer deferred its activation gradient).
    dz_amax: amax partials of dz (f16x2 scheme; computed here when missing).
    wt_image: the split image of W^T the recorded forward wrote next to W's (uint8, bf16x3); built here from ``weight``
    when missing (traced graphs, the one-plane schemes, direct calls)."""
    _f32(weight)
    _f32_or_bf16(scheme, dz, zmul)
    dz = dz.contiguous()
    B, Co, H, W = dz.shape
    Ci = weight.numel() // Co
    P = H * W
    gx = torch.empty(B, Ci, H, W, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dz.device)
    w2 = weight.reshape(Co, Ci).contiguous()
    wtsp = None
    if scheme != GEMM_EXACT:
        nbytes = lib.paradis_pw_gemm_split_bytes(Ci, Co, scheme)
        if wt_image is not None and wt_image.dtype == torch.uint8 and wt_image.numel() == nbytes:
            wtsp = wt_image
        else:
            wtsp = _split_image(weight, Co, Ci, True, scheme)[0]
    if scheme == GEMM_F16X2 and dz_amax is None:
        dz_amax = _amax_partials(dz)
    if zmul is not None:
        zmul = zmul.contiguous()
    io = (IO_X16 if _is16(dz) else 0) | (IO_Y16 if out_bf16 else 0) | (IO_Z16 if (x_act != 0 and _is16(zmul)) else 0)
    if io:
        if scheme != GEMM_BF16 or (_is16(dz) and (P % 8 or dz.data_ptr() % 16)):
            raise RuntimeError("bf16-stored gradients need the bf16-mixed GEMM scheme, H W % 8 == 0 and aligned planes")
        _lib.call("pw_gemm_dgrad", 2.0 * B * Co * Ci * P, dptr(wtsp), dptr(dz), dptr(zmul) if x_act != 0 else None,
                  dptr(gx), B, Co, Ci, P, Co * P, Ci * P, Ci * P, x_act, io, stream_ptr(), symbol="pw_gemm_dgrad16")
        return gx
    _lib.call("pw_gemm_dgrad", 2.0 * B * Co * Ci * P, dptr(w2), dptr(wtsp), scheme,
              dptr(dz_amax) if scheme == GEMM_F16X2 else None, dptr(dz),
              dptr(zmul) if x_act != 0 else None, None, dptr(gx), B, Co, Ci, P, Co * P, Ci * P, 0, Ci * P,
              x_act, stream_ptr())
    return gx


@_fake("pw_gemm_dgrad")
def _(dz, weight, zmul, x_act, dz_amax, scheme, wt_image=None, out_bf16=False):
    B, Co, H, W = dz.shape
    return dz.new_empty(B, weight.numel() // Co, H, W, dtype=torch.bfloat16 if out_bf16 else torch.float32)


@_define("pw_gemm_wgrad(Tensor dz, Tensor x, bool want_bias, Tensor? dz_amax, Tensor? x_amax, int scheme) "
         "-> (Tensor, Tensor)", autocast=((0, 1), 5))
def _pw_gemm_wgrad(dz, x, want_bias, dz_amax, x_amax, scheme):
    """gW[Co,Ci] = sum over samples and points of dz x^T; the bias gradient (row sums of dz) falls out
    of the same pass.  dz_amax / x_amax: amax partials (f16x2 scheme; computed here when missing)."""
    _f32_or_bf16(scheme, dz, x)
    dz = dz.contiguous()
    x, x_bs = _plane_view(x)
    B, Co, H, W = dz.shape
    Ci, P = x.shape[1], H * W
    gw = torch.empty(Co, Ci, dtype=torch.float32, device=dz.device)
    gb = torch.empty(Co if want_bias else 0, dtype=torch.float32, device=dz.device)
    ws = _ws(lib.paradis_pw_gemm_wgrad_ws_bytes(B, Co, Ci, P), dz.device)
    io = (IO_DY16 if _is16(dz) else 0) | (IO_X16 if _is16(x) else 0)
    if io:
        if P % 16 or dz.data_ptr() % 16 or x.data_ptr() % 16 or x_bs % 8:
            raise RuntimeError("bf16-stored GEMM operands need H W % 16 == 0 and 16-byte aligned planes")
        _lib.call("pw_gemm_wgrad", 2.0 * B * Co * Ci * P, dptr(dz), dptr(x), dptr(gw), dptr(gb) if want_bias else None,
                  B, Co, Ci, P, Co * P, x_bs, io, dptr(ws), stream_ptr(), symbol="pw_gemm_wgrad16")
        return gw, gb
    f16 = scheme == GEMM_F16X2
    if f16 and (dz_amax is None or dz_amax.numel() == 0):
        dz_amax = _amax_partials(dz)
    if f16 and (x_amax is None or x_amax.numel() == 0):
        x_amax = _amax_partials(x)
    _lib.call("pw_gemm_wgrad", 2.0 * B * Co * Ci * P, dptr(dz), dptr(x), dptr(gw), dptr(gb) if want_bias else None,
              B, Co, Ci, P, Co * P, x_bs, scheme, dptr(dz_amax) if f16 else None,
              dptr(x_amax) if f16 else None, dptr(ws), stream_ptr())
    return gw, gb


@_fake("pw_gemm_wgrad")
def _(dz, x, want_bias, dz_amax, x_amax, scheme):
    Co, Ci = dz.shape[1], x.shape[1]
    return dz.new_empty(Co, Ci, dtype=torch.float32), dz.new_empty(Co if want_bias else 0, dtype=torch.float32)


@_define("bias_grads(Tensor dz, bool want_bias, bool want_map) -> (Tensor, Tensor)", autocast=((0,), None))
def _bias_grads(dz, want_bias, want_map):
    """gb[Co] = sum over (B,H,W), gmap[Co,H,W] = sum over B of dz (fp32 sums; dz fp32, or bf16-stored in the bf16-mixed mode)."""
    _f32_or_bf16(GEMM_BF16, dz)
    dz = dz.contiguous()
    B, Co, H, W = dz.shape
    gb = torch.empty(Co if want_bias else 0, dtype=torch.float32, device=dz.device)
    gmap = torch.empty((Co, H, W) if want_map else (0,), dtype=torch.float32, device=dz.device)
    fn, name = (lib.paradis_bias_grads16, "bias_grads16") if _is16(dz) else (lib.paradis_bias_grads, "bias_grads")
    check(fn(dptr(dz), dptr(gmap) if want_map else None, dptr(gb) if want_bias else None, B, Co, H * W, Co * H * W,
             stream_ptr()), name)
    return gb, gmap


@_fake("bias_grads")
def _(dz, want_bias, want_map):
    B, Co, H, W = dz.shape
    return (dz.new_empty(Co if want_bias else 0, dtype=torch.float32),
            dz.new_empty((Co, H, W) if want_map else (0,), dtype=torch.float32))


def _pw_setup(ctx, inputs, output):
    x, weight, bias, bmap, residual, act, x_pre, x_act, defer, m8, pw, save_z, scheme, gate, _want_wt, out16 = inputs
    y, z, x_amax = output
    gated = gate is not None
    # (a gated epilogue blends with its residual: the backward needs both ends of the blend - the residual and the
    #  output, which the next block keeps alive anyway - and the gate)
    ctx.save_for_backward(x, weight, z, x_pre, m8, pw, x_amax, *((residual, y, gate) if gated else (None, None, None)))
    ctx.meta = (act, bias is not None, bmap is not None, residual is not None,
                x_act if x_pre is not None else 0, bool(defer), scheme)
    ctx.out16 = bool(out16)
    ctx.wt_image = _take_wt(weight)      # the W^T image this very forward call wrote (None: the dgrad builds its own)
    # z carries no gradient; without this autograd would materialise a full-size zero tensor for it
    ctx.mark_non_differentiable(z, x_amax)
    ctx.set_materialize_grads(False)


# ---- weight gradients on a side stream (round 6) -------------------------------------------------------------
# The weight-gradient GEMM of a pointwise layer depends on (dz, saved x) only; nothing of the dgrad chain waits for it
# (reference model/paradis.py:228-254: per-layer chain).  Issued on a second HIP stream it runs UNDER the memory- /
# VALU-bound kernels of the blocks that follow in backward (ChannelNorm, stencil, advection, blend) instead of in
# series with them.  Ordering contract:
#   * the side stream waits for an event recorded on the launching stream right after dz exists;
#   * dz / x / amax tensors are kept referenced until the launching stream has waited for the GEMM's completion event
#     (lagged by ``WgradSide.LAG`` launches, so that wait never stalls), so the caching allocator cannot hand their
#     blocks to later launching-stream kernels while the side stream still reads them - no ``record_stream`` (which a
#     graph capture would turn into memory held to the end of the capture);
#   * gW (and the fused bias gradient) are allocated ON the side stream; whoever consumes them on the launching stream
#     - autograd's AccumulateGrad (a pointer move while ``.grad`` is None), the optimiser, DDP's bucket copy - must be
#     ordered after the side stream: ``WgradSide.join()`` runs as an autograd-engine callback at the end of every
#     backward pass that used the side stream, and ``DelayedGrads`` (model/paradis.py) delivers the gradients of one
#     ADR layer to their AccumulateGrad nodes - hence to DDP's reducer hooks - one layer late, after a join of exactly
#     those launches.
class WgradSide:
    LAG = 6                    # launches kept in flight before the launching stream waits for the oldest
    enabled = ops._WGRAD_STREAM                 # PARADIS_WGRAD_STREAM
    PRIORITY = ops._WGRAD_STREAM_PRIORITY       # PARADIS_WGRAD_STREAM_PRIORITY: torch.cuda.Stream priority of the side stream
    _streams = {}              # device index -> torch.cuda.Stream
    _pending = []              # [(event, refs)] oldest first
    _callback_queued = False

    @classmethod
    def stream(cls, device) -> "torch.cuda.Stream":
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = cls._streams.get(idx)
        if st is None:
            st = cls._streams[idx] = torch.cuda.Stream(device=idx, priority=cls.PRIORITY)
        return st

    @classmethod
    def launch(cls, fn, dz, x, *rest):
        """run ``fn(dz, x, *rest)`` on the side stream, ordered after everything already enqueued on the current one"""
        side = cls.stream(dz.device)
        ready = torch.cuda.Event()
        ready.record()
        side.wait_event(ready)
        with torch.cuda.stream(side):
            out = fn(dz, x, *rest)
            done = torch.cuda.Event()
            done.record()
        cur = torch.cuda.current_stream()
        cls._pending.append((done, cur, (dz, x, rest)))
        while len(cls._pending) > cls.LAG:
            ev, st, _refs = cls._pending.pop(0)
            st.wait_event(ev)
        if not cls._callback_queued:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(cls.join)
                cls._callback_queued = True
            except RuntimeError:       # not inside a backward pass (a direct call of the backward op): join now
                cls.join()
        return out

    @classmethod
    def join(cls) -> None:
        """the current stream waits for every side-stream launch issued so far; references are dropped"""
        cls._callback_queued = False
        # (the engine runs its callbacks on a worker thread whose current stream is not the launching one: every entry
        #  remembers the stream it was launched from)
        for ev, st, _refs in cls._pending:
            st.wait_event(ev)
        cls._pending.clear()


def _pw_backward(ctx, saved, K, gy, gz=None, gamax=None):
    """``K``: name -> the OpOverload (OPS), or the kernel's Python function (RAW: an eager, un-traced backward; see
    ``_eager_front_end``)"""
    x, weight, z, x_pre, m8, pw, x_amax, res_saved, y_saved, gate = saved
    act, has_bias, has_map, has_res, x_act, deferred, scheme = ctx.meta
    need = ctx.needs_input_grad
    if gy is None:
        return (None,) * 16
    # the cotangent of a bf16-stored output arrives as bf16 (autograd keeps a gradient in its tensor's dtype); anything
    # else - a cast a caller put in between, an fp32 cotangent for a bf16 output - is brought to the dtype the kernels of
    # this node expect
    want = torch.bfloat16 if getattr(ctx, "out16", False) else torch.float32
    if gy.dtype != want:
        gy = gy.to(want)
    has_proj = pw is not None
    ggate = None
    if gate is not None:
        # gradient of the blend: d residual, d (activated GEMM output) - what the rest of this backward continues
        # with - and d gate, in one pass over (gy, residual, y)
        gres, gy, ggate = K["gated_blend_backward_out"](gy, res_saved, y_saved, gate)
        ggate = ggate.reshape(gate.shape)
    else:
        gres = gy if has_res else None
    if act != 0 and not deferred:
        # (bf16-mixed scheme: dz leaves the activation-gradient pass as a bf16 tensor - what its consumers, the two gradient
        #  GEMMs, round it to anyway - where their bf16-operand layout rules hold)
        dz16 = gy.dtype == torch.float32 and _stores_bf16(scheme, gy)
        dz = K["act_backward"](gy, z, act, dz16)
    else:
        dz = gy          # no activation, or the consumer already applied act'(z) (deferred)
    gx = gw = gb = gmap = gm8 = gpw = None
    # f16x2: one read pass over dz serves both of its GEMMs
    dz_amax = K["amax_partials"](dz) if (scheme == GEMM_F16X2 and (need[0] or need[1])) else None
    if need[0]:
        # (a bf16-stored input gets its gradient as bf16: with the activation-gradient hand-off that IS the producing
        #  layer's d(pre-activation), rounded to bf16 where the reference's autocast backward rounds it)
        gx = K["pw_gemm_dgrad"](dz, weight, x_pre if x_act != 0 else None, x_act, dz_amax, scheme,
                                getattr(ctx, "wt_image", None), x.dtype == torch.bfloat16)
    want_b = has_bias and need[2]
    want_p = has_proj and (need[9] or need[10])
    want_m = (has_map and need[3]) or want_p
    if need[1]:
        fused_b = want_b and not want_m     # bias gradient = row sums of dz: fused into the wgrad GEMM
        if K is RAW and WgradSide.enabled:
            gw, gbf = WgradSide.launch(K["pw_gemm_wgrad"], dz, x, fused_b, dz_amax, x_amax, scheme)
        else:
            gw, gbf = K["pw_gemm_wgrad"](dz, x, fused_b, dz_amax, x_amax, scheme)
        gw = gw.reshape(weight.shape)
        if fused_b:
            gb, want_b = gbf, False
    if want_b or want_m:
        gb2, gmap = K["bias_grads"](dz, want_b, want_m)
        if want_b:
            gb = gb2
        if not want_m:
            gmap = None
    if want_p:   # adjoint of the fused projection: gmap -> (gPw, gm8); the full map only lives here
        gpw, gm8 = K["global_bias_proj_backward"](gmap, m8, pw)
        gmap = None
    return gx, gw, gb, gmap, gres, None, None, None, None, gm8, gpw, None, None, ggate, None, None


# eager + recording calls take the same forward / setup / backward through a plain autograd.Function (``_core``).
# (dtypes were settled by ``pointwise``: fp32 everywhere except the bf16-stored activations of the bf16-mixed scheme - the
#  op has no blanket autocast rule, so nothing is widened here)
_PointwiseEager = _eager_front_end("pointwise", _pw_setup, _pw_backward, widen=False)


def pointwise(x, weight, bias=None, bias_map=None, residual=None, act=None, x_pre=None, x_act=None,
              defer_act_grad=False, bias_proj=None, scheme: Optional[int] = None, gate=None, out_bf16: bool = False):
    """y = residual + act(weight . x + bias[:,None] + bias_map); weight [Co,Ci] or [Co,Ci,1,1].

    ``bias_proj=(m8[Cin,H,W], Pw[Co,Cin])`` adds the projected low-rank GlobalBias map inside the GEMM
    epilogue instead of a materialised ``bias_map``.
    ``scheme``: GEMM arithmetic, default ``ops.GEMM_SCHEME`` (read when the call is made / traced); inside
    ``torch.autocast("cuda", dtype=torch.bfloat16)`` the default is ``GEMM_BF16`` (``autocast_scheme``).
    ``defer_act_grad=True`` returns ``(y, z)`` and expects the consumer to be another ``pointwise``
    called with ``x_pre=z, x_act=act`` (see the op docstring); only valid when ``y`` has no other use.
    ``gate`` [Co] (needs ``residual``): y = residual + sigmoid(gate) * (act(...) - residual), i.e.
    ``gated_blend(residual, pointwise(...), gate)`` without the intermediate tensor (bit-identical).
    ``out_bf16``: a REQUEST, honoured in the bf16-mixed scheme only (and only where the kernels' layout rules hold):
    y (and z) come back as ``torch.bfloat16`` tensors - what the reference's conv2d returns under autocast
    (model/blocks.py:86,110 with train.py:56) - for a consumer that is another ``pointwise``; the values are those of
    the fp32-stored result bit for bit.  A bf16 ``x`` / ``x_pre`` is consumed as stored in that scheme and widened to
    fp32 in every other."""
    if defer_act_grad and (act is None or residual is not None):
        raise ValueError("defer_act_grad needs an activation and no residual")
    if gate is not None and residual is None:
        raise ValueError("a gate needs the residual it blends with")
    m8, pw = bias_proj if bias_proj is not None else (None, None)
    require_hip(x, weight, bias, bias_map, residual, x_pre, m8, pw, gate)
    sch = autocast_scheme(ops.GEMM_SCHEME) if scheme is None else int(scheme)
    # dtypes (the op carries no blanket autocast rule): everything fp32, except that the bf16-mixed scheme consumes a
    # bf16-stored activation (and its pre-activation) as it is where the layout allows the 16-byte DMA
    ok16 = _stores_bf16(sch, x)
    if x.dtype != torch.float32 and not (ok16 and x.dtype == torch.bfloat16):
        x = x.float()
    if x_pre is not None and x_pre.dtype != torch.float32 and not (ok16 and x_pre.dtype == torch.bfloat16):
        x_pre = x_pre.float()
    weight, bias, bias_map, residual, m8, pw, gate = (
        t.float() if (t is not None and t.dtype != torch.float32) else t
        for t in (weight, bias, bias_map, residual, m8, pw, gate))
    # a bf16 output only where its gradient path exists: the consumer is a pointwise layer taking over the activation
    # gradient (recording), or nothing is recorded
    out16 = bool(out_bf16) and ok16 and residual is None and (bool(defer_act_grad) or not torch.is_grad_enabled())
    code = ACT_CODES[act]
    save_z = bool(defer_act_grad)
    if code != 0 and not save_z and torch.is_grad_enabled():
        save_z = any(t is not None and t.requires_grad for t in (x, weight, bias, bias_map, m8, pw))
    # (grad mode is off inside the op's own forward: the hint is computed here and travels as an argument)
    eager = not torch.compiler.is_compiling()
    want_wt = eager and torch.is_grad_enabled() and (x.requires_grad or (x_pre is not None and x_pre.requires_grad))
    args = (x, weight, bias, bias_map, residual, code, x_pre, ACT_CODES[x_act], bool(defer_act_grad), m8, pw,
            save_z, sch, gate, bool(want_wt), out16)
    # eager + recording: the plain autograd.Function front end (``_eager_front_end``).  Traced graphs keep the op.
    y, z, _ = _PointwiseEager.apply(*args) if (eager and torch.is_grad_enabled()) else _pointwise(*args)
    return (y, z) if defer_act_grad else y
