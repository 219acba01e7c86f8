"""torch custom ops (namespace ``paradis``) over the C-ABI HIP kernels.

Every entry point of the hot path is registered through ``torch.library``:

* a ``CUDA`` (= HIP on ROCm) kernel that launches the hand-written gfx950 kernels of
  ``libparadis_hip.so`` on the current HIP stream through the C ABI (no host sync);
* a fake (Meta) kernel giving the output shapes, so ``torch.compile(fullgraph=True)`` and
  AOTAutograd trace the model with these ops as opaque nodes (reference ``trainer.py:261-267``,
  ``model/paradis.py:195-206``);
* an autograd formula whose backward is again made of ``paradis::*_backward`` ops, so the traced
  backward graph contains no Python-only calls;
* an autocast rule: the kernels are fp32, under ``torch.autocast`` (the reference's
  ``precision="bf16-mixed"``, ``train.py:56``) inputs are cast to fp32 - never a narrower
  arithmetic than the reference's.

There is no CPU kernel: a CPU tensor raises (``_lib.require_hip`` / the dispatcher), and so does any
dtype but fp32.  The Python functions (``pointwise``, ``sl_advect`` ...) are thin wrappers that
check arguments and call ``torch.ops.paradis.*``.  Reference call sites are cited per op.

One module per op family, named after the ``csrc`` unit it drives; ``_core`` holds the registry and the dispatch policy
they share.  This file holds every process-wide setting, and everything is used as ``ops.<name>``.
"""
import os

from ._core import GEMM_BF16, GEMM_BF16X3, GEMM_EXACT, GEMM_F16X2

# ---------------------------------------------------------------------------
# Process-wide settings, each with the environment variable that gives its initial value.  They are plain attributes of
# THIS namespace: set them as ``ops.GEMM_SCHEME = ...``; the op families read ``ops.<NAME>`` when a call is made (or
# traced), never a copy taken at import.
# ---------------------------------------------------------------------------
# Arithmetic of the pointwise GEMMs (include/paradis_hip.h, a6), all fp32 in / accumulate / out:
#   "bf16x3" (default) three bf16 terms per operand value (an exact decomposition of the 24-bit significand with
#            fp32's exponent range per element), six products on the bf16 matrix pipe; error vs fp64 not above the
#            f32 MFMA chain's (tests/test_hip_gemm_split.py);
#   "exact"  the f32 MFMA chain (v_mfma_f32_32x32x2_f32);
#   "f16x2"  OPT-IN, not reference-width arithmetic: two f16 terms of the per-TENSOR scaled operands (a block-exponent
#            format: 22 significand bits relative to the tensor's largest magnitude), three products on the f16 pipe.
# PARADIS_GEMM selects ("split" = bf16x3, the name of earlier rounds).  The scheme is an explicit integer argument of
# the GEMM ops (as it is at the C ABI), so a traced graph pins the arithmetic it was traced with.
#   "bf16"   NOT fp32 arithmetic: the reference's bf16-mixed (AMP) training mode (train.py:56, use_amp: true) - operands
#            rounded to bf16, ONE product, fp32 accumulate, results rounded to bf16 where autocast's conv2d rounds them.
#            Selected by ``pointwise`` only inside ``torch.autocast(device_type="cuda", dtype=torch.bfloat16)`` (or by an
#            explicit ``scheme=``); PARADIS_GEMM cannot name it.
_SCHEMES = {"exact": GEMM_EXACT, "f16x2": GEMM_F16X2, "bf16x3": GEMM_BF16X3, "split": GEMM_BF16X3}


def _scheme_from_env() -> int:
    name = os.environ.get("PARADIS_GEMM", "bf16x3")
    if name not in _SCHEMES:
        raise ValueError(f"PARADIS_GEMM={name!r}: choose between {'|'.join(_SCHEMES)}")
    return _SCHEMES[name]


GEMM_SCHEME = _scheme_from_env()     # what the Python wrappers pass to the ops when the caller names no scheme
BF16_STORAGE = os.environ.get("PARADIS_BF16_STORAGE", "1") != "0"   # bf16-mixed scheme: chained activations as bf16 TENSORS (A/B switch)
# advection schedule hints applied when a call passes none (``ops.advect_flags``; diagnostics: tools/advect_halo_sweep.py)
ADVECT_FLAGS = int(os.environ.get("PARADIS_ADVECT_FLAGS", "0"), 0)
# weight images (ops/_images.py): ``with ops.frozen_weights():`` sets the first, ``ops.weights_updated()`` bumps the second
FROZEN_WEIGHTS = False
WEIGHT_EPOCH = 0
# weight gradients on a side stream (ops/gemm.py): what ``WgradSide.enabled`` / ``.PRIORITY`` start as; set those, not these
_WGRAD_STREAM = os.environ.get("PARADIS_WGRAD_STREAM", "0") == "1"
_WGRAD_STREAM_PRIORITY = int(os.environ.get("PARADIS_WGRAD_STREAM_PRIORITY", "0"))


def gemm_scheme_name() -> str:
    if GEMM_SCHEME == GEMM_BF16:
        return "bf16"
    return next(name for name, code in _SCHEMES.items() if code == GEMM_SCHEME)     # ("bf16x3" comes before its alias)


# ---------------------------------------------------------------------------
# The op families.  Importing one registers its ops; the order follows what each needs at import (``resample`` the
# stencil op).  What a backward formula reaches in another family (``gemm``'s: the blend, the GlobalBias projection) it
# looks up by name in OPS / RAW when it runs, so all families are imported here, before any call.
# ---------------------------------------------------------------------------
from . import _core, pad, advect, stencil, resample, norm, gbias, _images, gemm, elementwise, loss  # noqa: E402,I100

# Re-export: every name of every family, the private ``_<op>`` handles included (tests and tools call them), resolves as
# ``ops.<name>`` and is the same object.  The settings above are defined here alone - a family that bound one would
# have copied it at import.
_SETTINGS = ("GEMM_SCHEME", "BF16_STORAGE", "ADVECT_FLAGS", "FROZEN_WEIGHTS", "WEIGHT_EPOCH")
for _family in (_core, pad, advect, stencil, resample, norm, gbias, _images, gemm, elementwise, loss):
    _names = {k: v for k, v in vars(_family).items() if not k.startswith("__") and k != "_"}
    assert not set(_names).intersection(_SETTINGS), (_family.__name__, "binds a setting of the package")
    globals().update(_names)
