"""Plain fp64 references of the small streaming / reduction operations of include/paradis_hip.h.

Every function takes and returns ``torch.float64`` tensors on whatever device its inputs live on, is a direct
transcription of the mathematical definition (ATen ops only, gradients by autograd) and shares no code with the kernels
or with ``oracle/``.  tests/test_refs64_cpu.py pins them to the reference goldens and to the fp32 oracle; the GPU sweep
of tests/test_hip_kernel_edges.py measures the kernels against them.  The Muon / NorMuon step at the end is dtype-generic
and comes with the fp32 product orders that tests/test_hip_muon_edges.py uses as yardsticks."""
import math

import torch
import torch.nn.functional as F


def _f64(*ts):
    for t in ts:
        assert t is None or t.dtype == torch.float64, "the fp64 references take float64 tensors"


# ---------------------------------------------------------------------------------------------- resampling
def geocyclic_index(H, W, p, device=None):
    """Flat source index [(H+2p)*(W+2p)] of the geocyclic halo: longitude wraps; a row beyond a pole is the mirror image
    about the pole row (never duplicated) seen from the opposite meridian."""
    assert W % 2 == 0 and p <= H - 2
    i = torch.arange(-p, H + p, device=device).view(-1, 1)
    j = torch.arange(-p, W + p, device=device).view(1, -1) % W
    over = (i < 0) | (i >= H)
    row = torch.where(i < 0, -i, torch.where(i >= H, 2 * (H - 1) - i, i))
    col = torch.where(over, (j + W // 2) % W, j.expand(i.shape[0], -1))
    return (row * W + col).reshape(-1)


def avgpool_geo(x, stride):
    """Geocyclic 5x5 box mean with decimation: explicit pad by index map, then avg_pool2d.  x [..., H, W]."""
    _f64(x)
    H, W = x.shape[-2:]
    idx = geocyclic_index(H, W, 2, x.device)
    xp = x.reshape(-1, 1, H * W).index_select(2, idx).reshape(-1, 1, H + 4, W + 4)
    y = F.avg_pool2d(xp, kernel_size=5, stride=stride)
    return y.reshape(*x.shape[:-2], *y.shape[-2:])


def upsample_lonp(x, nlat, nlon):
    """Bilinear, align_corners, on the plane closed in longitude by its first column.  Written out tap by tap."""
    _f64(x)
    Hc, Wc = x.shape[-2:]
    sy = (Hc - 1) / (nlat - 1) if nlat > 1 else 0.0
    sx = Wc / nlon                                           # (Wc + 1 - 1) / (nlon + 1 - 1)
    fy = torch.arange(nlat, dtype=torch.float64, device=x.device) * sy
    fx = torch.arange(nlon, dtype=torch.float64, device=x.device) * sx
    y0 = fy.floor().clamp(0, Hc - 1).long()
    x0 = fx.floor().clamp(0, Wc - 1).long()
    y1 = (y0 + 1).clamp(max=Hc - 1)
    x1 = (x0 + 1) % Wc                                       # column Wc of the closed plane is column 0
    wy = (fy - y0).view(-1, 1)
    wx = fx - x0
    top = x[..., y0, :]
    bot = x[..., y1, :]
    rows = top * (1 - wy) + bot * wy
    return rows[..., x0] * (1 - wx) + rows[..., x1] * wx


# ---------------------------------------------------------------------------------------------- norm / bias
def channel_norm(x, weight, bias, eps=1e-5):
    """Per-pixel normalisation over the channel axis (-3), unbiased variance."""
    _f64(x, weight, bias)
    C = x.shape[-3]
    mean = x.sum(-3, keepdim=True) / C
    d = x - mean
    var = (d * d).sum(-3, keepdim=True) / (C - 1)
    return d / torch.sqrt(var + eps) * weight.view(-1, 1, 1) + bias.view(-1, 1, 1)


def global_bias_m8(A, U, V):
    """m8[c,h,w] = sum_r A[c,r] U[r,h] V[r,w]"""
    _f64(A, U, V)
    return ((A.unsqueeze(2) * U.unsqueeze(0)).transpose(1, 2).contiguous() @ V)   # [C,H,R] @ [R,W]


def global_bias_map(A, U, V, Pw=None):
    """map = m8, or Pw[Co,Cin] m8 with a projection"""
    m8 = global_bias_m8(A, U, V)
    if Pw is None:
        return m8
    _f64(Pw)
    Cin, H, W = m8.shape
    return (Pw @ m8.reshape(Cin, H * W)).reshape(-1, H, W)


# ---------------------------------------------------------------------------------------------- elementwise
def silu(x):
    _f64(x)
    return x / (1 + torch.exp(-x))


def gelu(x):
    _f64(x)
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def act(x, code):
    return {0: lambda t: t, 1: silu, 2: gelu}[code](x)


def gated_blend(h, adv, alpha):
    """h + sigmoid(alpha[c]) (adv - h), tensors [B,C,...]"""
    _f64(h, adv, alpha)
    s = 1 / (1 + torch.exp(-alpha))
    return h + s.view(1, -1, *([1] * (h.dim() - 2))) * (adv - h)


def bias_grads(dz):
    """dz [B,C,P] -> gmap[C,P] = sum_b, gbias[C] = sum_{b,p}"""
    _f64(dz)
    return dz.sum(0), dz.sum((0, 2))


# ---------------------------------------------------------------------------------------------- loss
def loss(pred, target, wf, wl, kind, delta):
    """mean(wf[c] wl[h] l(pred - target)) over [B,C,H,W]; kind 0: l = e^2; kind 1: the smooth reversed Huber
    (1 - s) delta |e| + s (e^2 + delta^2) / (2 delta), s = 1 / (1 + exp(-2 (|e| - delta)))."""
    _f64(pred, target, wf, wl)
    e = pred - target
    if kind == 0:
        l = e * e
    else:
        a = e.abs()
        s = 1 / (1 + torch.exp(-2 * (a - delta)))
        l = (1 - s) * (delta * a) + s * ((e * e + delta * delta) / (2 * delta))
    l = l * wf.view(1, -1, 1, 1)
    if wl is not None:
        l = l * wl.view(1, 1, -1, 1)
    return l.sum() / l.numel()


# ---------------------------------------------------------------------------------------------- AdamW
def adamw_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """One AdamW update in torch.optim.AdamW's operation order; returns the new (p, m, v).  ``step`` counts from 1."""
    _f64(p, g, m, v)
    p = p * (1 - lr * weight_decay)
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


# ---------------------------------------------------------------------------------------------- Muon / NorMuon
# Dtype-generic (the one exception to "float64 only" in this file): evaluated in float64 it is the reference of
# csrc/muon.hip, evaluated in float32 with one of the product orders below it is the yardstick "an ordinary fp32
# evaluation of the same algorithm" that tests/test_hip_muon_edges.py measures the kernels against.
NS_COEFFS = ((4.0848, -6.8946, 2.9270), (3.9505, -6.3029, 2.6377), (3.7418, -5.5913, 2.3037),
             (2.8769, -3.1427, 1.2046), (2.8366, -3.0525, 1.2012))


def matmul_k16(a, b):
    """a @ b with the k axis taken in chunks of 16 whose partial products are accumulated in order (the k depth of the
    MFMA tiles)"""
    a, b = a.contiguous(), b.contiguous()
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k in range(0, a.shape[1], 16):
        acc = acc + a[:, k:k + 16] @ b[k:k + 16]
    return acc


def matmul_seq(a, b):
    """a @ b strictly sequential over k: rank-1 updates, every product rounded before it is added (the least favourable
    ordinary order)"""
    a, b = a.contiguous(), b.contiguous()
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[k, None, :]
    return acc


def _bf16_terms(x):
    h = x.bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    return h, m, (r - m).bfloat16().float()


def matmul_bf16x3(a, b):
    """CPU emulation of the bf16x3 arithmetic (csrc/gemm_common.h): each fp32 operand is h + m + l in bfloat16 (round to
    nearest even, exact), the six partial products of weight >= 2^-16 are kept (m.m, l.h, h.l, m.h, h.m, h.h, smallest
    first, per 16-deep k tile) and accumulated in float32.  The products of two bfloat16 numbers are exact in float32."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    ah, am, al = _bf16_terms(a.contiguous())
    bh, bm, bl = _bf16_terms(b.contiguous())
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(0, a.shape[1], 16):
        s = slice(k, k + 16)
        for p, q in ((am, bm), (al, bh), (ah, bl), (am, bh), (ah, bm), (ah, bh)):
            acc = acc + p[:, s] @ q[s]
    return acc


def muon_momentum(g, m, mu, nesterov):
    """m <- mu m + g; returns (m_new, the matrix that is orthogonalised)"""
    m = mu * m + g
    return m, (g + mu * m if nesterov else m)


def newton_schulz(u, eps, matmul=torch.matmul, coeffs=NS_COEFFS):
    """Five quintic Newton-Schulz iterations on u / (||u||_F + eps), on the wide orientation; result in u's orientation"""
    tall = u.shape[0] > u.shape[1]
    x = u.mT if tall else u
    x = x / (x.norm() + eps)
    for a, b, c in coeffs:
        A = matmul(x, x.mT)
        B = b * A + c * matmul(A, A)
        x = a * x + matmul(B, x)
    return x.mT if tall else x


def muon_apply(w, x, v, *, lr, lr_adj, beta2, weight_decay):
    """The part of the step behind the orthogonalisation x: NorMuon's per-row second moment (v is not None; [rows, 1]),
    the rescale to the Frobenius norm x had, decoupled weight decay.  Returns (w_new, v_new, u)."""
    u = x
    if v is not None:
        norm_x = x.norm()
        v = beta2 * v + (1 - beta2) * (x * x).mean(dim=-1, keepdim=True)
        u = x / (v.sqrt() + 1e-8)
        u = u * (norm_x / u.norm().clamp(min=1e-8))
    return w * (1 - lr * weight_decay) - lr_adj * u, v, u


def muon_step(w, g, m, v, *, lr, lr_adj, mu, beta2, weight_decay, eps, nesterov, matmul=torch.matmul, coeffs=NS_COEFFS):
    """One Muon (v is None) or NorMuon (v: [rows, 1]) update of a [rows, cols] matrix; lr_adj is the shape-adjusted
    learning rate.  Returns (w_new, m_new, v_new, u), u = the orthogonalised update in the matrix's own orientation."""
    m, o = muon_momentum(g, m, mu, nesterov)
    w, v, u = muon_apply(w, newton_schulz(o, eps, matmul, coeffs), v, lr=lr, lr_adj=lr_adj, beta2=beta2,
                         weight_decay=weight_decay)
    return w, m, v, u
