"""What every op family shares: the ``paradis::`` registry and its dispatch policy (which calls may skip the dispatcher,
what autocast widens, the eager ``autograd.Function`` front end), the dtype / device checks, the small tensor helpers
and the constants that mirror ``include/paradis_hip.h``.  Process-wide settings are NOT here: they live in the package
namespace (``ops/__init__.py``) and are read as ``ops.<NAME>`` when a call is made."""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib
from .. import ops      # the package itself: settings are looked up on it at call time, never copied at import

ACT_CODES = {None: 0, "none": 0, "SiLU": 1, "GELU": 2}
MODE_CODES = {"bilinear": 1, "bicubic": 2}
# Arithmetic of the pointwise GEMMs (include/paradis_hip.h, a6; described where they are selected, ops/__init__.py)
GEMM_EXACT, GEMM_BF16, GEMM_F16X2, GEMM_BF16X3 = 0, 1, 2, 3
IO_X16, IO_Y16, IO_Z16, IO_DY16 = 1, 2, 4, 8       # include/paradis_hip.h PARADIS_IO_*: which tensors of a call are bf16
AMAX_PARTIALS = 1024

_DEF = torch.library.Library("paradis", "DEF")
OPS = {}            # op name -> OpOverload (torch.ops.paradis.<name>.default)
RAW = {}            # op name -> the Python function behind its HIP kernel (eager backward formulas call it directly)


# (private torch entry points, resolved once: if a torch build lacks them nothing is ever "plain" and every call takes
#  the dispatcher - slower, never wrong)
_dispatch_modes = getattr(torch._C, "_len_torch_dispatch_stack", None)
_functorch_top = getattr(getattr(torch._C, "_functorch", None), "peek_interpreter_stack", None)
_CAN_BE_PLAIN = _dispatch_modes is not None and _functorch_top is not None


def _plain(t) -> bool:
    """a real device tensor in an eager, un-traced call: the kernels' Python functions may be called directly (fake /
    functional / subclass tensors - FakeTensorMode, make_fx, torch.export - must go through the dispatcher)"""
    return (_CAN_BE_PLAIN and type(t) is Tensor and not torch.is_grad_enabled()
            and _dispatch_modes() == 0                    # make_fx(tracing_mode="real"), any TorchDispatchMode
            and _functorch_top() is None)                 # vmap / functional grad: plain-looking wrappers


def _all_plain(args) -> bool:
    """every tensor argument is a real ``Tensor`` / ``Parameter`` (no subclass or wrapper whose ``__torch_dispatch__`` the
    direct call would skip) and nothing watches the dispatcher"""
    if not (_CAN_BE_PLAIN and _dispatch_modes() == 0 and _functorch_top() is None):
        return False
    for a in args:
        if isinstance(a, Tensor) and type(a) is not Tensor and type(a) is not torch.nn.Parameter:
            return False
    return True


def _widen_for_autocast(args):
    """Inside ``torch.autocast`` the ops' autocast rule widens bf16 / fp16 tensor arguments to fp32 (the kernels are fp32).
    An eager ``autograd.Function`` front end sits ABOVE that rule, so it applies the rule itself before the kernel call
    AND before it saves anything for backward - a narrow saved input would reach the fp32-only backward kernels
    (tests/test_hip_amp.py::test_narrow_inputs_under_autocast_in_grad_mode).  Autograd casts the returned
    gradients back to the inputs' dtypes."""
    if not torch.is_autocast_enabled("cuda"):
        return args
    return tuple(a.float() if (isinstance(a, Tensor) and a.is_floating_point() and a.dtype != torch.float32) else a
                 for a in args)


def _eager_forward(name: str, args, settled: bool = False):
    """inside an ``autograd.Function.forward`` of an eager front end: the kernel's Python function directly where nothing
    watches the dispatcher and every tensor argument is a plain tensor, else the registered op.  Inside autocast the op
    it is (its autocast rule widens bf16 / fp16 inputs) unless the caller has ``settled`` the dtypes of ``args``."""
    if not torch.is_grad_enabled() and _all_plain(args) and (settled or not torch.is_autocast_enabled("cuda")):
        return RAW[name](*args)
    return OPS[name](*args)


def _eager_front_end(name: str, setup, backward, widen: bool):
    """Register ``setup`` / ``backward`` as the autograd formula of op ``name`` and return the same pair as a plain
    ``autograd.Function`` for eager recording calls: torch.library's generic autograd wrapper spends ~30 us per call of a
    15-argument op rebuilding the schema's argument list (torch/_library/utils.py fill_defaults; tools/host_profile.py:
    78 ``pointwise`` calls per step).  Traced graphs keep the op.

    ``backward(ctx, saved, K, *grads)`` gets the unpacked saved tensors and the table it calls its kernels through:
    ``OPS`` from the registered formula, always; from the eager one ``RAW`` - the kernels' Python functions, without the
    dispatcher -> autograd key -> autocast key -> Python kernel trip of ~12 us for each of ~250 op calls per training step,
    the arithmetic being the same code - where the cotangent and every saved tensor is plain.
    ``widen``: the op has the blanket autocast rule and its wrapper settles no dtypes, so the forward applies
    ``_widen_for_autocast`` itself; an op without it (``pointwise``) was handed settled dtypes by its wrapper."""
    _autograd(name, setup, lambda ctx, *grads: backward(ctx, ctx.saved_tensors, OPS, *grads))

    def forward(ctx, *args):
        if widen:
            args = _widen_for_autocast(args)
        out = _eager_forward(name, args, settled=not widen)
        setup(ctx, args, out)
        return out

    def eager_backward(ctx, *grads):
        saved = ctx.saved_tensors        # once: non-reentrant checkpointing unpacks (recomputes) on this access
        return backward(ctx, saved, RAW if (_plain(grads[0]) and _all_plain(saved)) else OPS, *grads)

    # (built with type() for the class name: autograd names the backward node after it)
    return type(f"_{name}_eager", (torch.autograd.Function,),
                {"forward": staticmethod(forward), "backward": staticmethod(eager_backward)})


def _selective_autocast(name: str, keep16: Tuple[int, ...], scheme_idx: Optional[int]) -> None:
    """Autocast rule of the pointwise-GEMM ops (round 6): widen every floating tensor argument to fp32 EXCEPT the
    bf16-stored activations / gradients at the positions ``keep16`` when the call's scheme (argument ``scheme_idx``; none
    = always) is the bf16-mixed one - there a bf16 tensor is the storage format the kernels consume, not something
    autocast has to undo (torch.library.register_autocast can only cast everything)."""
    op = getattr(torch.ops.paradis, name).default
    keyset = (torch._C.DispatchKeySet(torch._C.DispatchKey.AutocastCPU)
              | torch._C.DispatchKeySet(torch._C.DispatchKey.AutocastCUDA))

    def cast(args):
        mixed = scheme_idx is None or args[scheme_idx] == GEMM_BF16
        return tuple(a.float() if (isinstance(a, Tensor) and a.is_floating_point() and a.dtype != torch.float32
                                   and not (mixed and i in keep16 and a.dtype == torch.bfloat16)) else a
                     for i, a in enumerate(args))

    def py_impl(*args, **kwargs):
        assert not kwargs, "custom ops take positional arguments here"
        with torch._C._ExcludeDispatchKeyGuard(keyset):
            return op(*cast(args))

    try:
        op.py_impl(torch._C.DispatchKey.AutocastCUDA)(py_impl)
    except Exception:                      # (a torch without py_impl on OpOverload: the C++-side kernel below suffices)
        pass
    _DEF.impl(name, lambda _ks, *args, **kwargs: py_impl(*args, **kwargs), "AutocastCUDA", with_keyset=True)


def _define(schema: str, autocast=True):
    """Register ``schema`` in the ``paradis`` namespace with the decorated function as its HIP kernel.
    ``autocast``: True = every floating tensor argument is widened to fp32 under torch.autocast; a tuple
    ``(keep16 positions, scheme position or None)`` = the selective rule of ``_selective_autocast``; False = none."""
    name = schema[: schema.index("(")]
    _DEF.define(schema)

    def deco(fn):
        RAW[name] = fn
        _DEF.impl(name, fn, "CUDA")
        if autocast is True:
            torch.library.register_autocast(f"paradis::{name}", "cuda", torch.float32)
        elif autocast:
            _selective_autocast(name, tuple(autocast[0]), autocast[1])
        ov = getattr(torch.ops.paradis, name).default
        OPS[name] = ov
        return ov
    return deco


def _fake(name: str):
    """Register the fake (shape) kernel of an op."""
    return torch.library.register_fake(f"paradis::{name}")


def _autograd(name: str, setup, backward) -> None:
    torch.library.register_autograd(f"paradis::{name}", backward, setup_context=setup)


# Device check of the Python wrappers (the dtype check sits in the kernels, behind the autocast rule that widens
# bf16/fp16 inputs to fp32)
require_hip = functools.partial(_lib.require_hip, any_dtype=True)


def _f32(*tensors) -> None:
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"paradis_model_amd ops are fp32; got {t.dtype}")


def _f32_or_bf16(scheme: int, *tensors) -> None:
    """tensors that may be STORED as bf16 in the bf16-mixed scheme (round 6): GEMM activations, their pre-activations
    and the gradients of both; fp32 everywhere else"""
    for t in tensors:
        if t is not None and t.dtype != torch.float32 and not (t.dtype == torch.bfloat16 and scheme == GEMM_BF16):
            raise RuntimeError(f"paradis_model_amd ops are fp32 (bf16 tensors only in the bf16-mixed GEMM scheme); got {t.dtype}")


def _is16(t) -> bool:
    return t is not None and t.dtype == torch.bfloat16


def autocast_scheme(default: int) -> int:
    """GEMM arithmetic of a ``pointwise`` call that names none: inside ``torch.autocast("cuda", dtype=torch.bfloat16)`` -
    the reference's ``precision="bf16-mixed"`` (train.py:56; its shipped default, ``use_amp: true``) - the one-product
    bf16 scheme, i.e. what autocast makes of the reference's ``nn.Conv2d`` calls (model/blocks.py:86,110); the fp32
    scheme otherwise.  Everything else on the path (advection, stencils, norms) stays fp32 under autocast, as autocast
    keeps ``grid_sampler``; the scheme travels as an explicit argument of the op, so the backward and a traced graph
    use the arithmetic the forward was called with."""
    if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
        return GEMM_BF16
    return default


# ---- bf16-stored activations between a NON-GEMM producer and its pointwise consumer (round 6) ----------------------------
# ChannelNorm and the depthwise stencil can write their output as a bf16 tensor when its only consumer is a pointwise GEMM
# in the bf16-mixed scheme (``out_bf16``).  Autograd hands a bf16 tensor's producer a bf16 cotangent - the consumer's data
# gradient, bf16-valued in the reference's autocast backward as well (the gradient of conv2d's bf16 input).  The producers'
# backward kernels read it as it is stored where they have a bf16 instantiation (the streaming ChannelNorm backward, the
# whole-plane stencil backward: ``paradis_*_bwd16``); on every other path the op widens it first.  No side channel: the
# cotangent is an ordinary tensor, so checkpointing, hooks and foreign producers / consumers need no special case.
def _cotangent(gy, takes_bf16: bool):
    """the cotangent of a (possibly bf16-stored) output as the backward kernels of this node take it"""
    if gy is None or gy.dtype == torch.float32 or (takes_bf16 and gy.dtype == torch.bfloat16):
        return gy
    return gy.float()


def _stores_bf16(scheme: int, t: Tensor) -> bool:
    """THE wrapper-level rule for an activation (or its gradient) of ``t``'s grid travelling between two ops as a bf16
    tensor: the bf16-mixed scheme, the A/B switch ``ops.BF16_STORAGE``, and planes the 16-byte DMA of all three GEMM
    kernels can address (the kernels' own, differing layout checks stay with them)"""
    return scheme == GEMM_BF16 and ops.BF16_STORAGE and (t.shape[-2] * t.shape[-1]) % 16 == 0


def _want_bf16_out(x: Tensor, out_bf16: bool) -> bool:
    """a producer's ``out_bf16`` request is honoured where its consumer - a pointwise GEMM called next, inside the same
    autocast region - will run the bf16-mixed scheme and take a bf16 operand (see ``pointwise``)"""
    return bool(out_bf16) and _stores_bf16(autocast_scheme(ops.GEMM_SCHEME), x) and not torch.compiler.is_compiling()


def _ws(nbytes: int, device) -> Optional[Tensor]:
    if nbytes <= 0:
        return None
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def _planes_hw(x: Tensor) -> Tuple[int, int, int]:
    H, W = x.shape[-2:]
    return x.numel() // (H * W), H, W


def _plane_view(t: Tensor) -> Tuple[Tensor, int]:
    """[B,C,H,W] whose (H,W) planes are contiguous and channels are P apart (e.g. a channel slice of a
    larger contiguous tensor) is consumed in place: return (tensor, batch stride in elements);
    anything else is made contiguous."""
    B, C, H, W = t.shape
    if t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W:
        return t, (t.stride(0) if B > 1 else C * H * W)
    return t.contiguous(), C * H * W
