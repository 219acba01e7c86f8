"""GPU: the summation order of the streaming reductions is pinned (csrc/stream_common.h; DESIGN.md "Streaming
reductions: one layout").  For the two units whose partials are pure IEEE fp64 sums of exact products - ``clip.hip`` and
``stats.hip`` - the documented order is replayed in numpy float64 and the device's partials must equal it BIT FOR BIT
(compared as int64 views):

  * per thread t of a chunk the adds are strictly sequential over the iterations i, then over the cells k = 0..3 of the
    quad at 4 (256 i + t); the product of two fp32 values is exact in fp64, so a fused multiply-add and a multiply
    followed by an add give the same bits, and a cell past the end adds +0, which changes no bit;
  * the wave step is the xor tree o = 32, 16, .., 1 with v = v + v[lane ^ o];
  * the block step is (r0 + r1) + (r2 + r3) over the four waves;
  * the finishing kernel of ``stats.hip`` sums a group's chunk partials lane-strided (lane l: first + l, first + l + 64,
    ..), then the xor tree; the totals are the sum of the group sums in group order; columns 0..3 of ``out`` are their
    float32 roundings.

Sizes: every edge of the chunk walk (one cell, a part quad, one cell short of / exactly / one cell past a whole
iteration of 1024 cells and a whole chunk C, more than two chunks), once with 16-byte aligned tensors (the 16-byte loads)
and once with every tensor 4 bytes past a 16-byte boundary (the scalar loads).  Inputs as in tests/test_hip_stats.py:
seeded normals, the first and last element of every tensor and the element in front of every chunk edge times 2^10."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SPIKE = 1024.0


def _sizes(C):
    return [1, 3, 1023, 1024, 1025, C - 1, C, C + 1, 2 * C + 5]


def _draw(gen, n, C, scale=1.0):
    x = torch.randn(n, generator=gen) * scale
    pos = sorted({0, n - 1} | {k * C - 1 for k in range(1, (n + C - 1) // C + 1) if k * C - 1 < n})
    x[pos] *= SPIKE
    return x


def _device(t, offset):
    """a dense device copy; ``offset``: a view starting 4 bytes past a 16-byte boundary"""
    if t is None:
        return None
    if not offset:
        v = t.cuda()
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.zeros(t.numel() + 1, device="cuda")
    v = buf[1:].copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------------- the replay (numpy float64)
def _xor_tree(v):
    """v [..., 64] -> the wave's sum as every lane holds it after o = 32, 16, .., 1"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def _chunk_partials(a, b, ct, co, C):
    """partial[chunk] of sum a[t] * b[t] over the chunk (tensor ct, offset co); a / b: lists of float32 numpy arrays, an
    entry None = absent (the chunk's sum is 0)"""
    n_chunks = len(ct)
    prod = np.zeros((n_chunks, C), np.float64)
    for c, (t, off) in enumerate(zip(ct, co)):
        if a[t] is None or b[t] is None:
            continue
        x, y = a[t][off:off + C].astype(np.float64), b[t][off:off + C].astype(np.float64)
        prod[c, :x.size] = x * y                        # exact; cells past the end stay +0
    cells = prod.reshape(n_chunks, C // 1024, 256, 4)   # [chunk, iteration i, thread t, cell k]
    acc = np.zeros((n_chunks, 256), np.float64)
    for i in range(C // 1024):
        for k in range(4):
            acc = acc + cells[:, i, :, k]
    r = _xor_tree(acc.reshape(n_chunks, 4, 64))[:, :, 0]
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------- clip
@functools.lru_cache(maxsize=None)
def _clip_case(C):
    """(gradients on the CPU, one of them absent; the replayed partials): built once"""
    gen = torch.Generator().manual_seed(71)
    grads = [_draw(gen, n, C, 0.01) for n in _sizes(C)]
    grads.insert(4, None)                               # an absent gradient of C + 3 elements: two chunks of 0
    numels = [C + 3 if g is None else g.numel() for g in grads]
    ct = [t for t, n in enumerate(numels) for _ in range(0, n, C)]         # the table: tensor order, then offset
    co = [off for n in numels for off in range(0, n, C)]
    g_np = [None if g is None else g.numpy() for g in grads]
    return grads, numels, ct, _chunk_partials(g_np, g_np, ct, co, C)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned16", "offset4"])
def test_clip_partials_follow_the_documented_order(offset):
    from paradis_model_amd import _lib
    from paradis_model_amd.clip import ClipPlan
    C = _lib.lib.paradis_clip_grad_chunk()
    grads, numels, ct, want = _clip_case(C)
    plan = ClipPlan(numels, "cuda")
    assert plan.n_chunks == len(ct) == want.size
    plan.ws.fill_(float("nan"))
    dev = [_device(g, offset) for g in grads]
    plan.launch(dev, 1e30)                              # (nothing is clipped: the gradients stay as they are)
    got = plan.ws[:plan.n_chunks].cpu().numpy()
    absent = np.array([grads[t] is None for t in ct])
    assert absent.sum() == 2 and not got[absent].any() and not np.signbit(got[absent]).any()
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, [(int(c), ct[c], float(got[c]), float(want[c])) for c in bad[:8]]
    for g, d in zip(grads, dev):
        assert g is None or torch.equal(d.cpu(), g)


# ---------------------------------------------------------------------------------------------- stats
@functools.lru_cache(maxsize=None)
def _stats_case(C):
    gen = torch.Generator().manual_seed(72)
    spec = [(n, i % 2, True, True) for i, n in enumerate(_sizes(C))]
    spec.insert(3, (1030, 0, False, True))              # no gradient: its moment must not be read
    spec.insert(7, (2 * C - 3, 1, True, False))         # a gradient but no moment
    ps, gs, ms, groups = [], [], [], []
    for n, grp, has_g, has_m in spec:
        p, g = _draw(gen, n, C), _draw(gen, n, C, 0.01)
        m = 0.5 * g + 0.3 * _draw(gen, n, C, 0.01)
        ps.append(p)
        gs.append(g if has_g else None)
        ms.append(m if has_m else None)
        groups.append(grp)
    G = 2
    ct, co, first = [], [], [0] * (G + 1)               # the table: by group, then tensor, then offset
    for grp in range(G):
        first[grp] = len(ct)
        for t, p in enumerate(ps):
            if groups[t] == grp:
                ct += [t] * len(range(0, p.numel(), C))
                co += list(range(0, p.numel(), C))
    first[G] = len(ct)
    pn = [p.numpy() for p in ps]
    gn = [None if g is None else g.numpy() for g in gs]
    mn = [None if (m is None or g is None) else m.numpy() for m, g in zip(ms, gs)]
    part = np.stack([_chunk_partials(pn, pn, ct, co, C), _chunk_partials(gn, gn, ct, co, C),
                     _chunk_partials(gn, mn, ct, co, C), _chunk_partials(mn, mn, ct, co, C)], axis=1)     # [n_chunks, 4]
    # the finishing order: a wave per group, lane-strided over the group's chunks, the xor tree; totals in group order
    rows = np.zeros((G + 1, 4), np.float64)
    for g in range(G):
        lanes = np.zeros((64, 4), np.float64)
        for i in range(first[g], first[g + 1]):
            lanes[(i - first[g]) % 64] = lanes[(i - first[g]) % 64] + part[i]
        rows[g] = _xor_tree(lanes.T)[:, 0]
    tot = np.zeros(4, np.float64)
    for g in range(G):
        tot = tot + rows[g]
    rows[G] = tot
    return ps, gs, ms, groups, G, part, rows.astype(np.float32)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned16", "offset4"])
def test_stats_partials_and_sums_follow_the_documented_order(offset):
    from paradis_model_amd import _lib
    from paradis_model_amd.diagnostics import StatsPlan
    C = _lib.lib.paradis_param_stats_chunk()
    ps, gs, ms, groups, G, want, want_rows = _stats_case(C)
    plan = StatsPlan([p.numel() for p in ps], groups, G, "cuda")
    assert plan.n_chunks == want.shape[0]
    plan.ws.fill_(float("nan"))
    plan.out.fill_(float("nan"))
    out = plan.launch([_device(p, offset) for p in ps], [_device(g, offset) for g in gs],
                      [_device(m, offset) for m in ms])
    got = plan.ws[:4 * plan.n_chunks].view(plan.n_chunks, 4).cpu().numpy()
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, [(int(c), int(j), float(got[c, j]), float(want[c, j])) for c, j in bad[:8]]
    rows = out[:, :4].cpu().numpy()
    assert np.array_equal(np.ascontiguousarray(rows).view(np.int32), np.ascontiguousarray(want_rows).view(np.int32)), \
        (rows, want_rows)
