"""What the layout of ``paradis_model_amd/ops/`` - one module per op family, settings in the package namespace - could
break without any other test noticing.  No kernel is launched.

* the op schemas (what a traced or exported graph names) and the sets of ops with ``Autograd`` / ``AutocastCUDA`` kernels
  equal ``tests/golden/ops_schemas.json``, recorded once from the commit before the split by

      import json, torch
      from paradis_model_amd import ops
      has = torch._C._dispatch_has_kernel_for_dispatch_key
      doc = {"schemas": {n: str(ops.OPS[n]._schema) for n in sorted(ops.OPS)},
             "autograd": sorted(n for n in ops.OPS if has(f"paradis::{n}", "Autograd")),
             "autocast_cuda": sorted(n for n in ops.OPS if has(f"paradis::{n}", "AutocastCUDA"))}
      json.dump(doc, open("tests/golden/ops_schemas.json", "w"), indent=1, sort_keys=True)

* a setting assigned as ``ops.<NAME> = ...`` reaches a traced call (a family module that copied it at import would not
  see the assignment);
* ``frozen_weights`` / ``weights_updated`` write the package's settings;
* every name that tests, tools and the rest of the package use resolves on ``ops``, the ``ops._<op>`` handles as the
  registered ops themselves."""
import json
import os

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from paradis_model_amd import ops
from tests._util import make_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_schemas.json")


def _has(name, key):
    return torch._C._dispatch_has_kernel_for_dispatch_key(f"paradis::{name}", key)


def test_schemas_and_kernel_sets_are_those_recorded_before_the_split():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want["schemas"]) == 40 and len(want["autograd"]) == 17 and len(want["autocast_cuda"]) == 38
    assert {n: str(op._schema) for n, op in ops.OPS.items()} == want["schemas"]
    assert sorted(n for n in ops.OPS if _has(n, "Autograd")) == want["autograd"]
    assert sorted(n for n in ops.OPS if _has(n, "AutocastCUDA")) == want["autocast_cuda"]
    assert set(ops.RAW) == set(ops.OPS)


def _traced_args(fn, inputs, target):
    """arguments of the single ``target`` node in the graph ``torch.compile(fn, fullgraph=True)`` captures"""
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    torch._dynamo.reset()
    torch.compile(fn, backend=backend, fullgraph=True)(*inputs)
    assert len(graphs) == 1, "graph break"
    (node,) = [n for n in graphs[0].graph.nodes if n.op == "call_function" and str(n.target) == target]
    return node.args


def test_gemm_scheme_assigned_on_the_package_reaches_a_traced_pointwise():
    keep = ops.GEMM_SCHEME
    try:
        with FakeTensorMode(allow_non_fake_inputs=True):
            x, w = torch.empty(2, 8, 8, 16, device="cuda"), torch.empty(4, 8, device="cuda")
            for scheme in (ops.GEMM_EXACT, ops.GEMM_F16X2):
                ops.GEMM_SCHEME = scheme
                args = _traced_args(lambda x, w: ops.pointwise(x, w), (x, w), "paradis.pointwise.default")
                assert (ops.GEMM_EXACT, ops.GEMM_F16X2) == (0, 2) and args[12] == scheme
    finally:
        ops.GEMM_SCHEME = keep
        torch._dynamo.reset()


def test_advect_flags_assigned_on_the_package_reach_a_traced_advection():
    H, W, K = 8, 16, 3
    _, lg, og = make_grid(H, W, False)
    geom = ops.AdvectGeometry(lg, og)
    assert geom.separable and ops.ADVECT_SEPARABLE == 4 and ops.advect_flags(halo=3) == 1024
    keep = ops.ADVECT_FLAGS
    try:
        with FakeTensorMode(allow_non_fake_inputs=True):
            f, vel = torch.empty(2, K, H, W, device="cuda"), torch.empty(2, 2 * K, H, W, device="cuda")
            for flags, want in ((0, 4), (ops.advect_flags(halo=3), 1028)):      # ADVECT_SEPARABLE is ORed in
                ops.ADVECT_FLAGS = flags
                args = _traced_args(lambda f, vel: ops.sl_advect_vel(f, vel, geom, 0.1), (f, vel),
                                    "paradis.sl_advect_vel.default")
                assert args[-1] == want
    finally:
        ops.ADVECT_FLAGS = keep
        torch._dynamo.reset()


def test_frozen_weights_and_weights_updated_write_the_package_settings():
    assert ops.FROZEN_WEIGHTS is False
    with ops.frozen_weights():
        assert ops.FROZEN_WEIGHTS is True
        ops._IMAGES["sentinel"] = None
        with ops.frozen_weights(False):
            assert ops.FROZEN_WEIGHTS is False
        assert ops.FROZEN_WEIGHTS is True
    assert ops.FROZEN_WEIGHTS is False and not ops._IMAGES
    epoch = ops.WEIGHT_EPOCH
    ops.weights_updated()
    assert ops.WEIGHT_EPOCH == epoch + 1


# every ``ops.<name>`` used by tests/, tools/, bench.py, __graft_entry__.py and the rest of the package
WRAPPERS = ["geocyclic_pad", "sl_advect", "sl_advect_vel", "dwconv_geo", "dwconv_geo_skip", "avgpool_geo", "upsample_lonp",
            "channel_norm", "channel_norm_skip", "global_bias_map", "global_bias_m8", "pointwise", "activation",
            "gated_blend", "add", "add_bias_map", "concat_channels", "paradis_loss", "amse_loss", "amse_tables",
            "amse_grid_check", "AdvectGeometry", "advect_flags", "frozen_weights", "weights_updated", "gemm_scheme_name",
            "autocast_scheme", "require_hip", "WgradSide"]
CONSTANTS = ["ACT_CODES", "MODE_CODES", "GEMM_EXACT", "GEMM_BF16", "GEMM_F16X2", "GEMM_BF16X3", "IO_X16", "IO_Y16",
             "IO_Z16", "IO_DY16", "AMAX_PARTIALS", "ADVECT_GENERIC", "ADVECT_TILED", "ADVECT_SEPARABLE", "ADVECT_TILES",
             "ADVECT_STRIPS", "OPS", "RAW", "_SCHEMES", "_IMAGES", "_BOX_WEIGHTS", "_AMSE_TABLES"]
SETTINGS = ["GEMM_SCHEME", "ADVECT_FLAGS", "BF16_STORAGE", "FROZEN_WEIGHTS", "WEIGHT_EPOCH"]
HELPERS = ["_scheme_from_env", "_plain", "_want_bf16_out", "_geom_args", "_ensure_step_hook", "_version_of", "_take_wt",
           "dptr", "stream_ptr", "lib"]
OP_HANDLES = ["avgpool_geo", "avgpool_geo_backward", "upsample_lonp", "upsample_lonp_backward", "global_bias_map",
              "global_bias_m8_backward", "global_bias_proj_backward", "channel_norm", "channel_norm_backward",
              "gated_blend", "gated_blend_backward", "gated_blend_backward_out", "dwconv_geo", "dwconv_geo_dgrad",
              "dwconv_geo_dgrad_add", "dwconv_geo_wgrad", "dwconv_geo_bwd", "act_backward", "pw_gemm_wgrad",
              "amax_partials", "sl_advect_vel", "sl_advect_vel_backward"]


def test_every_name_used_outside_the_package_resolves_on_ops():
    for name in WRAPPERS + CONSTANTS + SETTINGS + HELPERS:
        assert hasattr(ops, name), name
    for name in OP_HANDLES:
        assert getattr(ops, "_" + name) is ops.OPS[name], name
    # dicts and classes are shared by identity with the module that uses them
    assert ops.WgradSide is ops.gemm.WgradSide and ops._IMAGES is ops._images._IMAGES
    assert ops.OPS is ops._core.OPS and ops.RAW is ops._core.RAW and ops._BOX_WEIGHTS is ops.resample._BOX_WEIGHTS
    for name in ("enabled", "LAG", "PRIORITY"):
        assert hasattr(ops.WgradSide, name), name
