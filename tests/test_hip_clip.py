"""GPU: the multi-tensor global-norm clip ``paradis_clip_grad_norm`` (csrc/clip.hip) against plain fp64 at its dispatch
edges - tensor sizes around the quad, the 1024-cell iteration and the chunk; separate allocations (16-byte loads and stores)
and views one element into a larger buffer (4-byte aligned: scalar path); an absent tensor; more chunks than the finishing
workgroup has threads; no chunks; all-zero gradients; a NaN; two runs to the same bits - and ``clip.clip_grad_norm_`` on
module parameters whose gradient addresses change between calls.

Bounds (derived, not measured): the sum of squares is formed in double from exact products, at most 2^26 non-negative
additions contribute <= 2^-27 relative, the one rounding to fp32 contributes 2^-24: |out[0] - norm64| <= 2^-23 norm64, and
the same for the coefficient.  The scale pass is one IEEE fp32 multiply per element: ``torch.equal``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
GUARD = 7.25                       # what the cells around the views hold: must never change


def _chunk():
    from paradis_model_amd import _lib
    return _lib.lib.paradis_clip_grad_chunk()


def _sizes():
    C = _chunk()
    return [1, 3, 4, 5, 1023, 1024, 1025, C - 1, C, C + 1, 2 * C + 5]


ABSENT = 5                         # index in the tensor list whose address is 0 (a tensor of 77 cells)


def _make(placement, scale, seed=0, sizes=None):
    """(tensors on the device, backing buffer or None): seeded randn * scale; index ABSENT is inserted as an absent tensor"""
    sizes = list(sizes if sizes is not None else _sizes())
    sizes.insert(ABSENT, 77)
    g = torch.Generator().manual_seed(seed)
    vals = [(torch.randn(n, generator=g) * scale) for n in sizes]
    if placement == "separate":
        ts = [v.cuda() for v in vals]
        assert all(t.data_ptr() % 16 == 0 for t in ts)
        return ts, None
    # views: tensor i starts one element behind a multiple of four cells of one buffer -> address = 4 mod 16
    offs, total = [], 0
    for n in sizes:
        offs.append(total + 1)
        total += (n + 1 + 3) // 4 * 4 + 4
    buf = torch.full((total,), GUARD, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ts = []
    for v, o in zip(vals, offs):
        t = buf[o:o + v.numel()]
        t.copy_(v)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        ts.append(t)
    return ts, buf


def _guards_intact(buf, ts):
    mask = torch.ones_like(buf, dtype=torch.bool)
    base = buf.data_ptr()
    for t in ts:
        o = (t.data_ptr() - base) // 4
        mask[o:o + t.numel()] = False
    return bool((buf[mask] == GUARD).all())


def _norm64(ts, skip=ABSENT):
    s = torch.zeros((), dtype=torch.float64, device="cuda")
    for i, t in enumerate(ts):
        if i != skip:
            s += t.double().square().sum()
    return float(s.sqrt())


def _run(plan, ts, max_norm, absent=ABSENT):
    grads = [None if i == absent else t for i, t in enumerate(ts)]
    return plan.launch(grads, max_norm).clone()


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e25])
@pytest.mark.parametrize("placement", ["separate", "views"])
def test_clip_kernel_at_dispatch_edges(placement, scale):
    from paradis_model_amd.clip import ClipPlan
    ts, buf = _make(placement, scale)
    plan = ClipPlan([t.numel() for t in ts], "cuda")
    before = [t.clone() for t in ts]
    n64 = _norm64(ts)
    assert 0.0 < n64 < 3e38                                      # representable in fp32 (an fp32 sum of squares is not at 1e25)
    # ---- max_norm = 2 norm: nothing is clipped, nothing changes
    out = _run(plan, ts, 2.0 * n64)
    assert abs(float(out[0]) - n64) <= EPS * n64, (float(out[0]), n64)
    assert float(out[1]) == 1.0
    assert all(torch.equal(a, b) for a, b in zip(ts, before))
    # ---- max_norm = norm / 2: every present gradient is g * out[1], one exact multiply
    max_norm = 0.5 * n64
    out = _run(plan, ts, max_norm)
    c64 = max_norm / (n64 + 1e-6)
    assert torch.isfinite(out).all()
    assert abs(float(out[0]) - n64) <= EPS * n64, (float(out[0]), n64)
    assert abs(float(out[1]) - c64) <= EPS * c64, (float(out[1]), c64)
    assert float(out[1]) < 1.0
    for i, (a, b) in enumerate(zip(ts, before)):
        if i == ABSENT:
            assert torch.equal(a, b)                            # address 0: neither read nor written
        else:
            assert torch.equal(a, b * out[1]), i
            assert torch.isfinite(a).all()
    if buf is not None:
        assert _guards_intact(buf, ts)
    # ---- determinism: the same input again gives the same bits
    for t, b in zip(ts, before):
        t.copy_(b)
    first = [t.clone() for t in ts]
    out2 = _run(plan, ts, max_norm)
    assert torch.equal(out2, out)
    for i, (a, b) in enumerate(zip(ts, first)):
        assert torch.equal(a, b if i == ABSENT else b * out[1])


def test_aligned_and_view_placements_give_the_same_bits():
    from paradis_model_amd.clip import ClipPlan
    a, _ = _make("separate", 1.0, seed=3)
    b, _ = _make("views", 1.0, seed=3)
    plan = ClipPlan([t.numel() for t in a], "cuda")
    m = 0.5 * _norm64(a)
    oa, ob = _run(plan, a, m), _run(plan, b, m)
    assert torch.equal(oa, ob)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_more_chunks_than_finishing_threads():
    """3,000 tensors of 1..7 elements carved from one buffer: 3,000 chunks for a finishing workgroup of 1,024 threads"""
    from paradis_model_amd.clip import ClipPlan
    g = torch.Generator().manual_seed(11)
    sizes = [1 + i % 7 for i in range(3000)]
    buf = torch.randn(sum(sizes), generator=g).cuda()
    ts = list(buf.split(sizes))
    assert len({t.data_ptr() % 16 for t in ts}) > 1            # both paths
    plan = ClipPlan(sizes, "cuda")
    assert plan.n_chunks == 3000
    before = buf.clone()
    n64 = float(before.double().square().sum().sqrt())
    out = plan.launch(ts, 0.5 * n64).clone()
    c64 = 0.5 * n64 / (n64 + 1e-6)
    assert abs(float(out[0]) - n64) <= EPS * n64 and abs(float(out[1]) - c64) <= EPS * c64
    assert torch.equal(buf, before * out[1])


def test_no_chunks_absent_everywhere_and_zero_gradients():
    from paradis_model_amd.clip import ClipPlan
    empty = ClipPlan([], "cuda")
    assert empty.n_chunks == 0
    empty.out.fill_(-3.0)
    assert empty.launch([], 1.0).tolist() == [0.0, 1.0]
    zero_sized = ClipPlan([0, 0], "cuda")                      # tensors without elements: no chunks either
    zero_sized.out.fill_(-3.0)
    e = torch.empty(0, device="cuda")
    assert zero_sized.launch([e, e], 1.0).tolist() == [0.0, 1.0]
    plan = ClipPlan([5, 1025], "cuda")
    plan.out.fill_(-3.0)
    assert plan.launch([None, None], 2.5).tolist() == [0.0, 1.0]
    zs = [torch.zeros(5, device="cuda"), torch.zeros(1025, device="cuda")]
    assert plan.launch(zs, 2.5).tolist() == [0.0, 1.0]
    assert all(bool((z == 0).all()) for z in zs)


@pytest.mark.parametrize("placement", ["separate", "views"])
def test_one_nan_poisons_norm_coefficient_and_every_present_gradient(placement):
    from paradis_model_amd.clip import ClipPlan
    ts, buf = _make(placement, 1.0, seed=5)
    keep = ts[ABSENT].clone()
    ts[7][1000] = float("nan")
    plan = ClipPlan([t.numel() for t in ts], "cuda")
    out = _run(plan, ts, 1.0)
    assert torch.isnan(out).all()
    for i, t in enumerate(ts):
        if i == ABSENT:
            assert torch.equal(t, keep)
        else:
            assert torch.isnan(t).all(), i
    if buf is not None:
        assert _guards_intact(buf, ts)


def test_clip_grad_norm_on_module_parameters_follows_new_addresses():
    from paradis_model_amd import clip
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).cuda()
    model[1].bias.requires_grad_(False)                       # a parameter without a gradient is skipped
    params = list(model.parameters())
    x = torch.randn(9, 33, device="cuda")

    def backward(scale):
        (model(x).square().sum() * scale).backward()
        grads = [p.grad for p in params]
        return grads, [None if g is None else g.clone() for g in grads]

    def expect(raw, out):
        return [None if g is None else g * out[1] for g in raw]

    def n64(raw):
        return float(sum(g.double().square().sum() for g in raw if g is not None).sqrt())

    g1, raw1 = backward(1.0)
    out1 = clip.clip_grad_norm_(params, 0.5 * n64(raw1)).clone()
    assert abs(float(out1[0]) - n64(raw1)) <= EPS * n64(raw1) and float(out1[1]) < 1.0
    assert params[3].grad is None
    want1 = expect(raw1, out1)
    assert all(w is None or torch.equal(p.grad, w) for p, w in zip(params, want1))
    # new state and new gradient tensors behind the same parameters (the old ones are kept alive: other addresses)
    model.load_state_dict({k: v * 0.5 for k, v in model.state_dict().items()})
    model.zero_grad(set_to_none=True)
    g2, raw2 = backward(3.0)
    assert all(a is None or a.data_ptr() != b.data_ptr() for a, b in zip(g1, g2))
    out2 = clip.clip_grad_norm_(params, 0.5 * n64(raw2)).clone()
    assert abs(float(out2[0]) - n64(raw2)) <= EPS * n64(raw2)
    assert all(w is None or torch.equal(p.grad, w) for p, w in zip(params, expect(raw2, out2)))
    assert all(w is None or torch.equal(g, w) for g, w in zip(g1, want1))       # the first call's tensors: untouched
    # what the plan refuses
    plan = clip.ClipPlan([p.numel() for p in params], "cuda")
    grads = [p.grad for p in params]
    w = torch.randn(33, 65, device="cuda")
    with pytest.raises(RuntimeError, match="non-contiguous"):
        plan.launch([w.t()] + grads[1:], 1.0)
    with pytest.raises(RuntimeError, match="fp32"):
        plan.launch([grads[0].double()] + grads[1:], 1.0)
    with pytest.raises(RuntimeError, match="cpu"):
        plan.launch([grads[0].cpu()] + grads[1:], 1.0)
    with pytest.raises(ValueError, match="elements"):
        plan.launch([grads[1]] + grads[1:], 1.0)
    with pytest.raises(ValueError, match="max_norm"):
        plan.launch(grads, 0.0)
