"""Plain fp64 references of the small streaming / reduction operations of include/paradis_hip.h.

Every function takes and returns ``torch.float64`` tensors on whatever device its inputs live on, is a direct
transcription of the mathematical definition (ATen ops only, gradients by autograd) and shares no code with the kernels
or with ``oracle/``.  tests/test_refs64_cpu.py pins them to the reference goldens and to the fp32 oracle; the GPU sweep
of tests/test_hip_kernel_edges.py measures the kernels against them."""
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
