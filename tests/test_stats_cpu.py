"""CPU: the host side of the training diagnostics - tests/stats_oracle.py against hand-computed cases, the new C-ABI
symbols and their argument rejection before any HIP call, the parameter groups of ``diagnostics.TrainStats`` against the
reference's eight keys, the chunk table of ``paradis_param_stats`` and the ``on_step`` hook of ``harness.rollout_loss``."""
import ctypes
import math

import pytest
import torch

from paradis_model_amd.config import reduced_config, stub_datamodule
from tests import stats_oracle as SO
from tests._util import make_grid

REFERENCE_KEYS = ["advection", "alpha_adv", "diffusion", "input_proj", "output_proj", "reaction", "static_encoder",
                  "velocity_nets"]


def _t(*v):
    return torch.tensor(v, dtype=torch.float32)


# ================================================================================================ the oracle
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("seq", [False, True])
def test_oracle_group_without_gradients_is_absent(dtype, seq):
    named = [("model.a.w", _t(3, 4)), ("model.b.w", _t(1, 1))]
    logged, sums = SO.metrics(named, [_t(6, 8), None], [_t(3, 4), _t(9, 9)], dtype, seq)
    assert set(logged) == {"grad/total", "grad/a", "gradratio/a", "pnorm/a", "grad_alignment/a", "grad_alignment/total"}
    assert logged["grad/a"] == 10.0 and logged["pnorm/a"] == 5.0 and logged["gradratio/a"] == 2.0
    assert logged["grad/total"] == 10.0
    assert abs(logged["grad_alignment/a"] - 1.0) <= 1e-6 and abs(logged["grad_alignment/total"] - 1.0) <= 1e-6
    assert sums["a"] == (25.0, 100.0, 50.0, 25.0)
    assert sums["b"] == (2.0, 0.0, 0.0, 0.0)             # the moment of a parameter without a gradient is not read
    assert sums["total"] == (27.0, 100.0, 50.0, 25.0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_oracle_gradients_without_moments_give_no_alignment_but_count_in_the_totals(dtype):
    named = [("model.a.w", _t(3, 4)), ("model.c.w", _t(0))]
    logged, sums = SO.metrics(named, [_t(3, 4), _t(12)], [_t(4, -3), None], dtype)
    assert set(logged) == {"grad/total", "grad/a", "gradratio/a", "pnorm/a", "grad_alignment/a", "grad/c", "gradratio/c",
                           "pnorm/c", "grad_alignment/total"}
    assert logged["grad/total"] == 13.0                                  # sqrt(25 + 144): group c counts
    assert logged["grad/c"] == 12.0
    assert abs(logged["pnorm/c"] - 1e-12) <= 1e-18                       # clamp_min(eps)
    assert abs(logged["gradratio/c"] - 12.0 / logged["pnorm/c"]) <= 1e-6 * logged["gradratio/c"]
    assert logged["grad_alignment/a"] == 0.0 and logged["grad_alignment/total"] == 0.0      # orthogonal, but present
    assert sums["c"] == (0.0, 144.0, 0.0, 0.0) and sums["total"] == (25.0, 169.0, 0.0, 25.0)


def test_oracle_two_tensors_per_group_and_first_step():
    named = [("model.a.w", _t(1, 2, 2)), ("model.a.frozen", _t(4)), ("model.b.w", _t(2))]
    grads = [_t(2, 0, 0), None, _t(1.5)]
    logged, sums = SO.metrics(named, grads, [_t(1, 0, 0), _t(100), _t(-2)])
    assert logged["pnorm/a"] == 5.0 and logged["grad/a"] == 2.0 and logged["gradratio/a"] == 0.4
    assert abs(logged["grad_alignment/a"] - 1.0) <= 1e-11 and abs(logged["grad_alignment/b"] + 1.0) <= 1e-11
    assert logged["grad/total"] == 2.5
    assert abs(logged["grad_alignment/total"] - (-1.0 / (2.5 * math.sqrt(5.0) + 1e-12))) <= 1e-15
    assert sums["a"] == (25.0, 4.0, 2.0, 1.0) and sums["total"] == (29.0, 6.25, -1.0, 5.0)
    # the first optimiser step: no state yet, no alignment key at all
    first, _ = SO.metrics(named, grads, [None, None, None])
    assert set(first) == {"grad/total", "grad/a", "gradratio/a", "pnorm/a", "grad/b", "gradratio/b", "pnorm/b"}
    # no gradient anywhere: grad/total = 0 and nothing else
    none, s0 = SO.metrics(named, [None] * 3, [None] * 3)
    assert none == {"grad/total": 0.0} and s0["total"] == (29.0, 0.0, 0.0, 0.0)


# ================================================================================================ the C ABI
def test_param_stats_symbols_and_argument_rejection_before_any_hip_call():
    from paradis_model_amd import _lib
    L = _lib.lib
    for name in ("paradis_param_stats_chunk", "paradis_param_stats_ws_bytes", "paradis_param_stats"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert len(_lib.SIGNATURES["paradis_param_stats"][1]) == 11
    assert L.paradis_abi_version() == 10
    C = L.paradis_param_stats_chunk()
    assert C >= 1024 and C % 4 == 0
    for n in (0, 1, 7, 2000):
        assert L.paradis_param_stats_ws_bytes(n) >= 32 * n
    assert L.paradis_param_stats_ws_bytes(-1) == 0
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first, or has n_groups == 0

    def call(ptrs=fake, numel=fake, ct=fake, co=fake, gfc=fake, T=2, chunks=3, G=2, ws=fake, out=fake):
        return L.paradis_param_stats(ptrs, numel, ct, co, gfc, T, chunks, G, ws, out, None)

    assert call(G=0) == 0                                            # no groups: accepted, nothing to do
    assert call(G=0, ptrs=None, numel=None, ct=None, co=None, gfc=None, ws=None, out=None) == 0
    for kw in (dict(T=-1), dict(chunks=-1), dict(G=-1)):
        assert call(**kw) == 1 and "counts" in _lib.last_error()
    assert call(gfc=None) == 1 and "group_first_chunk" in _lib.last_error()
    for kw in (dict(ptrs=None), dict(numel=None), dict(ct=None), dict(co=None)):
        assert call(**kw) == 1 and "tables" in _lib.last_error()
    assert call(out=None) == 1 and "result" in _lib.last_error()
    assert call(ws=None) == 1 and "workspace" in _lib.last_error()
    assert call(T=0) == 1 and "no tensor" in _lib.last_error()
    assert call(G=100000) == 1 and "groups" in _lib.last_error()


def test_param_stats_and_trainstats_refuse_cpu_tensors():
    from paradis_model_amd.diagnostics import param_stats
    x = torch.zeros(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        param_stats([x], [x], [x], [0])


# ================================================================================================ groups
class _Wrap(torch.nn.Module):
    def __init__(self, attr, inner):
        super().__init__()
        setattr(self, attr, inner)


def _reduced_model():
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = reduced_config()
    lat_deg, lg, og = make_grid(16, 32, False)
    torch.manual_seed(42)
    return Paradis(stub_datamodule(cfg), cfg, lg, og), build_loss(cfg, lat_deg)


def test_trainstats_group_keys_are_the_reference_keys():
    from paradis_model_amd.diagnostics import TrainStats, group_key
    model, loss = _reduced_model()
    bare = TrainStats(model, loss)
    assert bare.group_keys == REFERENCE_KEYS
    # the reference: name.split(".")[1] of LitParadis.named_parameters(), whose names start with "model."
    want = [("model." + n).split(".")[1] for n, _ in model.named_parameters()]
    assert [bare.group_keys[g] for g in bare.groups] == want
    assert len(bare.groups) == len(list(model.parameters()))
    for wrapped in (_Wrap("module", model), _Wrap("_orig_mod", model), _Wrap("module", _Wrap("_orig_mod", model)),
                    _Wrap("_orig_mod", _Wrap("module", model))):
        names = [n for n, _ in wrapped.named_parameters()]
        assert names[0].startswith(("module.", "_orig_mod."))
        ts = TrainStats(wrapped, loss)
        assert ts.group_keys == REFERENCE_KEYS and ts.groups == bare.groups
    assert group_key("module._orig_mod.input_proj.layers.0.weight") == "input_proj"
    assert group_key("alpha_adv") == "alpha_adv"
    assert group_key("static_encoder._orig_mod.proj.weight") == "static_encoder"
    assert bare.channel_names == list(loss.output_name_order)
    assert TrainStats(model, loss, channel_losses=False).channel_names == []


def test_chunk_table_is_sorted_by_group_and_covers_every_element_once():
    from paradis_model_amd import _lib
    from paradis_model_amd.diagnostics import chunk_table
    C = _lib.lib.paradis_param_stats_chunk()
    numels = [1, 3, C - 1, C, C + 1, 2 * C + 5, 0, 7]
    groups = [2, 0, 1, 2, 0, 1, 2, 3]                    # interleaved: the table has to sort; group 4 owns nothing
    G = 5
    ct, co, first = chunk_table(numels, groups, G, C)
    assert len(ct) == len(co) == sum((n + C - 1) // C for n in numels) == 1 + 1 + 1 + 1 + 2 + 3 + 0 + 1
    assert len(first) == G + 1 and first[0] == 0 and first[G] == len(ct) and first == sorted(first)
    assert first[4] == first[5]                          # the empty group
    chunk_groups = [groups[t] for t in ct]
    assert chunk_groups == sorted(chunk_groups)
    for g in range(G):
        assert all(groups[t] == g for t in ct[first[g]:first[g + 1]])
    covered = [torch.zeros(n, dtype=torch.int32) for n in numels]
    for t, off in zip(ct, co):
        assert off % C == 0 and 0 <= off < numels[t]
        covered[t][off:min(off + C, numels[t])] += 1
    assert all(bool((c == 1).all()) for c in covered)
    with pytest.raises(ValueError):
        chunk_table([4, 4], [0, 5], 2, C)
    with pytest.raises(ValueError):
        chunk_table([4, 4], [0], 2, C)


# ================================================================================================ the rollout hook
def test_rollout_loss_on_step_hook_sees_every_step_and_leaves_the_loss_alone():
    from paradis_model_amd.harness import make_grids, rollout_loss, synthetic_batch
    from tests.test_distributed_cpu import OracleLoss, OracleReplica
    cfg = reduced_config()
    lat_deg, lg, og = make_grids(16, 32, False)
    model, loss_fn = OracleReplica(cfg, lg, og), OracleLoss(cfg, lat_deg)
    S = 2
    batch = synthetic_batch(16, 32, False, 1, S, seed=5)
    seen = []
    with torch.no_grad():
        plain, outs = rollout_loss(model, loss_fn, batch, num_common=83, n_inputs=2, backward=False, keep_outputs=True)
        hooked, _ = rollout_loss(model, loss_fn, batch, num_common=83, n_inputs=2, backward=False,
                                 on_step=lambda out, tgt: seen.append((out.detach().clone(), tgt)))
    assert torch.equal(plain, hooked)
    assert len(seen) == S == len(outs)
    for s, (out, tgt) in enumerate(seen):
        assert torch.equal(out, outs[s])
        assert tgt.shape == batch[1][:, s].shape and tgt.data_ptr() == batch[1][:, s].data_ptr()
        assert torch.equal(tgt, batch[1][:, s])


def test_trainstep_takes_a_stats_object_and_defaults_to_none():
    import inspect
    from paradis_model_amd.harness import TrainStep, rollout_loss
    assert inspect.signature(TrainStep.__init__).parameters["stats"].default is None
    assert inspect.signature(rollout_loss).parameters["on_step"].default is None
