"""Cases, inputs and cached CPU references of the Muon / NorMuon step, shared by tests/test_refs64_cpu.py (which holds the
fp32 yardsticks under the ceiling, without a GPU) and tests/test_hip_muon_edges.py (which measures csrc/muon.hip against
them).  Everything here is CPU work; the expensive part of a reference - the Newton-Schulz iteration in fp64 and in the
four fp32 product orders of tests/_refs64.py - is computed once per matrix and kept for the session."""
import numpy as np
import torch

from tests import _refs64 as R


def f32(x):
    """the value the C ABI's `float` argument receives"""
    return float(np.float32(x))


LR, LR_ADJ, MU, BETA2, WD, EPS = f32(5e-3), f32(0.02), f32(0.95), f32(0.95), f32(0.01), f32(1e-8)
CEILING = 1e-5                       # the project's forward ceiling (SURVEY.md 8c ii)
SCALES = (1.0, 2.0 ** 10, 2.0 ** -10)      # gradient magnitude of member 0, 1, 2 of a stack: a norm partial read from the
                                           # neighbouring matrix changes the normalisation by 2^10

# name, rows, cols, T, nesterov.  Each shape is the smallest that selects its branch of csrc/muon.hip / the bgemm path
# (blocks(n) = min(ceil(n / 256), 1024) workgroups of 256 threads; GEMM tiles 128 x 128, k depth 16; transpose tiles 32 x 32).
CASES = [
    # n = 40 < 256: one partial workgroup; M = 1 in every product; cols < 64 in normuon_rows_kernel (one partial wave)
    ("1x40", 1, 40, 1, False),
    # transposed (rows > cols); cols = 1: a one-element row per block of normuon_rows_kernel, strided by cs = K = 40
    ("40x1", 40, 1, 1, True),
    # n = 1023: four workgroups, the last one ragged by one element; transposed; partial 32 x 32 transpose tiles both ways;
    # batch stride n % 4 != 0 (LDS-DMA kernel ineligible: M = 31)
    ("33x31", 33, 31, 1, False),
    # every product on the register-staged exact kernel: K % 16 != 0 (20) and M % 16 != 0 (8)
    ("8x20", 8, 20, 1, True),
    # every product eligible for the LDS-DMA exact kernel (pd_exact_dma_eligible); square: not transposed
    ("64x64", 64, 64, 1, False),
    # LDS-DMA eligible with K != M: products [64,96]x[96,64], [64,64]x[64,64], [64,64]x[64,96]
    ("64x96", 64, 96, 1, True),
    # 300 partials and 300 rows: second trip of block_sum_fixed (i += 256) in normalize and apply; cols = 256 exactly (one
    # full trip of normuon_rows_kernel); transposed; product 1 staged (K = 300), products 2 and 3 LDS-DMA (M = 256)
    ("300x256", 300, 256, 1, False),
    # n = 266760 > 262144: second, ragged sweep of every grid-stride loop; M * M = 263169: second sweep of muon_poly_kernel;
    # 1024 partials (four trips of block_sum_fixed); 513 = 4 x 128 + 1 = 16 x 32 + 1: one-row ragged GEMM and transpose
    # tiles; cols = 520: three trips of normuon_rows_kernel, the last ragged
    ("513x520", 513, 520, 1, True),
    # the same, transposed: strided reads in muon_apply_kernel and normuon_rows_kernel, three block_sum_fixed trips over rows
    ("520x513", 520, 513, 1, False),
    # stacks (blockIdx.y = matrix): the group sits at columns 2..4 of a table with stride 7
    ("33x31 T3", 33, 31, 3, True),       # batch strides n = 1023 and mm = 961, neither a multiple of 4
    ("64x96 T3", 64, 96, 3, False),      # LDS-DMA kernel with batch strides
    ("513x520 T3", 513, 520, 3, True),   # partials of matrix t at part + t * 1024; second sweeps with blockIdx.y > 0
]
CASE = {c[0]: c for c in CASES}

ORDERS = {"matmul": torch.matmul, "k16": R.matmul_k16, "seq": R.matmul_seq, "bf16x3": R.matmul_bf16x3}


def orders_of(split):
    """the fp32 evaluations that count as yardstick for an arithmetic of the kernel"""
    return ("matmul", "k16", "seq", "bf16x3") if split else ("matmul", "k16", "seq")


_inputs, _orth = {}, {}


def inputs(rows, cols, member):
    """fp32 CPU inputs of member `member` of a stack of [rows, cols] matrices: w, g, m (non-zero), v (positive, of the
    size rowmean(x^2) has for an orthogonalised x)"""
    key = (rows, cols, member)
    if key not in _inputs:
        gen = torch.Generator().manual_seed(1000 * rows + 10 * cols + member)
        s = SCALES[member]
        _inputs[key] = dict(w=torch.randn(rows, cols, generator=gen) * 0.1,
                            g=torch.randn(rows, cols, generator=gen) * s,
                            m=torch.randn(rows, cols, generator=gen) * (2 * s),
                            v=(torch.rand(rows, 1, generator=gen) + 0.5) / max(rows, cols))
    return _inputs[key]


def orth(rows, cols, member, nesterov):
    """m64 and the orthogonalisation of the step's momentum: "x64" in fp64, and one fp32 evaluation per product order"""
    key = (rows, cols, member, nesterov)
    if key not in _orth:
        i = inputs(rows, cols, member)
        m64, o64 = R.muon_momentum(i["g"].double(), i["m"].double(), MU, nesterov)
        out = dict(m64=m64, x64=R.newton_schulz(o64, EPS))
        _, o32 = R.muon_momentum(i["g"], i["m"], MU, nesterov)
        for name, mm in ORDERS.items():
            out[name] = R.newton_schulz(o32, EPS, mm)
        _orth[key] = out
    return _orth[key]


def refs(rows, cols, member, nesterov, normuon, w_zero, v_zero=False, lr=LR, lr_adj=LR_ADJ):
    """fp64 (w, v) of one step and the same per fp32 product order: dict(w64, v64, m64, cpu={order: (w, v)})"""
    i, o = inputs(rows, cols, member), orth(rows, cols, member, nesterov)
    w = torch.zeros_like(i["w"]) if w_zero else i["w"]
    v = (torch.zeros_like(i["v"]) if v_zero else i["v"]) if normuon else None
    kw = dict(lr=lr, lr_adj=lr_adj, beta2=BETA2, weight_decay=WD)
    w64, v64, _ = R.muon_apply(w.double(), o["x64"], None if v is None else v.double(), **kw)
    cpu = {name: R.muon_apply(w, o[name], v, **kw)[:2] for name in ORDERS}
    return dict(w64=w64, v64=v64, m64=o["m64"], cpu=cpu)


def err(got, ref):
    """max|got - ref| / max|ref| of one matrix"""
    return float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def matrices():
    """the distinct (rows, cols, member, nesterov) of CASES"""
    seen = []
    for _, rows, cols, T, nesterov in CASES:
        for t in range(T):
            if (rows, cols, t, nesterov) not in seen:
                seen.append((rows, cols, t, nesterov))
    return seen
