"""CPU restatement of the AMSE loss (reference utils/amse_loss.py) and of the spherical-harmonic transform it calls
(torch_harmonics.RealSHT on the "equiangular" grid, norm="backward"), in fp64 or fp32.

The transform is restated from torch_harmonics' published algorithm (the package is not a dependency):
* nodes: colatitudes pi*j/(nlat-1), both poles, Clenshaw-Curtis weights on cos(theta) by Waldvogel's construction;
* longitude: X_m = 2 pi * rfft(x, norm="forward"), m < nlon//2 + 1;
* Legendre: orthonormal associated Legendre functions with the Condon-Shortley phase by the three-term recurrence of
  torch_harmonics' legpoly, in fp64, times SHT_NORM_FACTOR (the "backward" normalisation: sqrt(4 pi), unpinned);
* coefficients c[l, m] = sum_j w_j P_l^m(cos theta_j) X_m(theta_j), l < nlat.
``tables(nlat, ms)`` builds the weighted Legendre table for a subset of orders, so the 721 x 1440 table can be checked
without building all of it.

``sht(..., dft="matrix")`` takes the longitude transform as a product with a twiddle table (the algorithm of sht.hip: a
direct DFT accumulates nlon terms, an FFT log nlon, so in fp32 it is the fairer yardstick), ``cc_weights_cosine`` is
the closed cosine form of the Clenshaw-Curtis rule that sht.hip evaluates, and ``edge_fields`` / ``edge_reference``
are the inputs and the CPU figures of the tile-edge tests (tests/test_hip_amse_edges.py, tests/test_amse_cpu.py).
"""
import functools
import math

import numpy as np
import torch

SHT_NORM_FACTOR = math.sqrt(4.0 * math.pi)
EPS = 1e-7


def cc_weights(n):
    """(cos theta nodes from -1 to 1, Clenshaw-Curtis weights) - Waldvogel (2006), as torch_harmonics computes them"""
    tcc = np.cos(np.linspace(np.pi, 0, n))
    n1 = n - 1
    N = np.arange(1, n1, 2)
    l_ = len(N)
    m_ = n1 - l_
    v = np.concatenate([2 / N / (N - 2), 1 / N[-1:], np.zeros(m_)])
    v = 0 - v[:-1] - v[-1:0:-1]
    g0 = -np.ones(n1)
    g0[l_] += n1
    g0[m_] += n1
    g = g0 / (n1 ** 2 - 1 + (n1 % 2))
    w = np.fft.ifft(v + g).real
    return tcc, np.concatenate((w, w[:1]))


def cc_weights_cosine(n):
    """(cos theta nodes from 1 to -1, weights) in the closed cosine form that sht.hip's cc_nodes_kernel evaluates:
    w_j = c_j / n1 * (1 - sum_{k=1}^{n1 // 2} b_k cos(2 k theta_j) / (4 k^2 - 1)), n1 = n - 1, theta_j = pi j / n1,
    c_j = 1 at the two poles and 2 between them, b_k = 1 where 2 k = n1 and 2 elsewhere"""
    n1 = n - 1
    th = np.pi * np.arange(n) / n1
    k = np.arange(1, n1 // 2 + 1)
    bk = np.where(2 * k == n1, 1.0, 2.0)
    s = (bk * np.cos(2.0 * k * th[:, None]) / (4.0 * k * k - 1.0)).sum(1)
    cj = np.full(n, 2.0)
    cj[0] = cj[-1] = 1.0
    return np.cos(th), cj / n1 * (1.0 - s)


def colatitudes(nlat):
    cost, _ = cc_weights(nlat)
    return np.flip(np.arccos(cost)).copy()


def legendre_order(m, lmax, theta, norm_factor=SHT_NORM_FACTOR):
    """P[l - m, j] for l = m .. lmax-1 of order m (Condon-Shortley phase included), fp64; the same recurrence and
    operation order as torch_harmonics' legpoly (diagonal chain, first off-diagonal, three-term recurrence in l)"""
    x = np.cos(theta)
    pmm = np.full_like(x, norm_factor / np.sqrt(4 * np.pi))
    for l in range(1, m + 1):
        pmm = np.sqrt((2 * l + 1) * (1 + x) * (1 - x) / 2 / l) * pmm
    out = np.zeros((max(lmax - m, 0), len(x)))
    if lmax <= m:
        return out
    out[0] = pmm
    if m + 1 < lmax:
        out[1] = np.sqrt(2 * (m + 1) + 1) * x * pmm
    for l in range(m + 2, lmax):
        out[l - m] = (x * np.sqrt((2 * l - 1) / (l - m) * (2 * l + 1) / (l + m)) * out[l - m - 1]
                      - np.sqrt((l + m - 1) / (l - m) * (2 * l + 1) / (2 * l - 3) * (l - m - 1) / (l + m)) * out[l - m - 2])
    if m % 2 == 1:
        out = -out
    return out


def tables(nlat, ms=None, lmax=None):
    """{m: weighted table [lmax - m, nlat]} (fp64); lmax defaults to nlat - 1 (the degrees AMSE reads)"""
    lmax = nlat - 1 if lmax is None else lmax
    ms = range(lmax) if ms is None else ms
    _, w = cc_weights(nlat)
    th = colatitudes(nlat)
    return {int(m): legendre_order(int(m), lmax, th) * w[None, :] for m in ms}


@functools.lru_cache(maxsize=2)
def dense_weights(nlat, nlon):
    """torch_harmonics' dense layout [mmax, lmax, nlat] (lmax = nlat, mmax = nlon//2 + 1), fp64 (cached: read-only)"""
    lmax, mmax = nlat, nlon // 2 + 1
    t = tables(nlat, range(min(mmax, lmax)), lmax)
    out = np.zeros((mmax, lmax, nlat))
    for m, tab in t.items():
        out[m, m:] = tab
    return torch.from_numpy(out)


class RealSHT(torch.nn.Module):
    """restated torch_harmonics.RealSHT (equiangular grid only): x [..., nlat, nlon] -> complex [..., nlat, nlon//2+1]"""

    def __init__(self, nlat, nlon, grid="equiangular", norm="backward", csphase=True):
        super().__init__()
        if grid != "equiangular" or norm != "backward" or not csphase:
            raise NotImplementedError("only the equiangular grid with norm='backward' is restated")
        self.nlat, self.nlon, self.lmax, self.mmax = nlat, nlon, nlat, nlon // 2 + 1
        self.register_buffer("weights", dense_weights(nlat, nlon).float(), persistent=False)

    def legendre(self, xre, xim):
        w = self.weights.to(xre.dtype)
        re = torch.einsum("...km,mlk->...lm", xre, w)
        im = torch.einsum("...km,mlk->...lm", xim, w)
        return torch.complex(re, im)

    def forward(self, x):
        assert x.shape[-2] == self.nlat and x.shape[-1] == self.nlon
        x = 2.0 * torch.pi * torch.fft.rfft(x, dim=-1, norm="forward")
        x = torch.view_as_real(x[..., : self.mmax])
        return self.legendre(x[..., 0], x[..., 1])


def dft_table(nlon, mmax):
    """[nlon, 2 mmax] fp64: 2 pi / nlon * (cos, -sin)(2 pi (m i mod nlon) / nlon), the phase reduced exactly (sht.hip's
    twiddle table, for every order the restated transform keeps)"""
    i = np.arange(nlon)[:, None]
    m = np.arange(mmax)[None, :]
    ang = 2 * np.pi * ((i * m) % nlon) / nlon
    return torch.from_numpy(np.concatenate([np.cos(ang), -np.sin(ang)], 1) * (2 * np.pi / nlon))


def sht(x, dtype=torch.float64, dft="fft"):
    """coefficients [..., nlat, nlon//2+1] of x in `dtype` arithmetic (fp64: the accuracy yardstick).  dft="fft" is the
    transform as torch_harmonics takes it; dft="matrix" forms X_m as x @ dft_table (built in fp64, cast to `dtype`)."""
    m = RealSHT(x.shape[-2], x.shape[-1])
    if dtype == torch.float64:
        m.weights = dense_weights(x.shape[-2], x.shape[-1])
    x = x.to(dtype)
    if dft == "fft":
        return m(x)
    if dft != "matrix":
        raise ValueError(f"dft must be 'fft' or 'matrix', got {dft!r}")
    tab = dft_table(m.nlon, m.mmax).to(dtype)
    return m.legendre(x @ tab[:, :m.mmax], x @ tab[:, m.mmax:])


def amse_from_coeffs(pc, tc):
    """AMSE of coefficient arrays [B, C, lmax, mmax] (vectorised restatement of the reference's loops)"""
    K = pc.shape[-2] - 1
    M = pc.shape[-1]
    pk, tk = pc[..., :K, :], tc[..., :K, :]
    k = torch.arange(K).view(K, 1)
    m = torch.arange(M).view(1, M)
    wgt = torch.where(m <= k, torch.where(m == 0, 1.0, 2.0), 0.0).to(pc.real.dtype)
    psd_p = (wgt * pk.abs() ** 2).sum(-1) + EPS
    psd_t = (wgt * tk.abs() ** 2).sum(-1) + EPS
    cross = (wgt * (torch.conj(pk) * tk)).sum(-1)
    coh = torch.clamp(cross.abs() / (torch.sqrt(psd_p * psd_t + EPS) + EPS), 0.0, 1.0)
    per = (torch.sqrt(psd_p) - torch.sqrt(psd_t)) ** 2 + 2.0 * torch.max(psd_p, psd_t) * (1.0 - coh)
    return per.mean(-1).mean()


def amse(pred, target, dtype=torch.float64, dft="fft"):
    """scalar AMSE (unweighted); NaN -> 1e6 as the reference"""
    loss = amse_from_coeffs(sht(pred, dtype, dft), sht(target.detach(), dtype, dft))
    if torch.isnan(loss):
        return torch.tensor(1e6, dtype=loss.dtype)
    return loss


def synth(nlat, nlon, modes, dtype=torch.float64):
    """a field [nlat, nlon] whose coefficients are `modes` {(l, m): complex} (the inverse transform of the restated basis).
    The analysis gives them back, to rounding, at every degree l' with l + l' <= nlat - 1: there the Clenshaw-Curtis rule
    integrates the product of the two Legendre functions exactly."""
    th = colatitudes(nlat)
    phi = 2 * np.pi * np.arange(nlon) / nlon
    f = np.zeros((nlat, nlon))
    for (l, m), c in modes.items():
        P = legendre_order(m, l + 1, th)[l - m] / (4 * np.pi)        # orthonormal / sqrt(4 pi), then / sqrt(4 pi)
        c = complex(c)
        scale = 1.0 if m == 0 else 2.0
        f += scale * P[:, None] * (c.real * np.cos(m * phi) - c.imag * np.sin(m * phi))[None, :]
    return torch.from_numpy(f).to(dtype)


def value_and_grad(pred, target, dtype=torch.float64, dft="fft"):
    """(AMSE as a float, d AMSE / d pred in fp64) evaluated in `dtype` arithmetic on the CPU"""
    pr = pred.detach().to(dtype).clone().requires_grad_(True)
    v = amse(pr, target.detach().to(dtype), dtype, dft)
    v.backward()
    return float(v.detach()), pr.grad.double()


# ---- inputs and CPU figures of the tile-edge tests ---------------------------------------------------------------------
# (H, B, C), W = 2 (H - 1), N = B C, M = H - 1: the edges of sht.hip's 64 x 64 x 16 GEMM tile under its four index mappings
# (DftFwd rows 2M, cols H N, depth W; LegFwd per m rows M - m, cols 4N, depth H; LegAdj rows H, cols 2N, depth M - m;
# DftAdj rows H N, cols W, depth 2M), of amse_spectral_kernel's 256-plane blocks and amse_finish_kernel's stride of 256
EDGE_CASES = [
    (9, 1, 1),      # one plane
    (9, 1, 16),     # 4N = 64: exactly one LegFwd column tile
    (9, 1, 17),     # 4N = 68: a second column tile of 4, the target's imaginary block straddles a tile
    (9, 3, 11),     # N = 33, 2N = 66: LegAdj gets a second column tile of 2; B > 1 and C > 1
    (9, 2, 128),    # N = 256: one full spectral block and one full finish pass
    (9, 1, 257),    # one plane in spectral block 1 and one in the finish kernel's second pass
    (3, 1, 5),      # the smallest legal grid: M = 2, W = 4 < TK, order 1 has a single row
    (4, 1, 5),      # even H; legendre_table_kernel's `m + 1 >= M` return fires at m = 2
    (65, 1, 5),     # M = 64: the LegFwd row tile exactly full at m = 0; 2M = 128 puts the cos / sin split on a tile
                    # boundary; LegAdj rows 65 = a second tile of one row; depth H = 65 = 4 TK + 1
    (66, 1, 17),    # even H; M = 65: a second row tile of ONE row at m = 0, empty for every m >= 1 (the early return);
                    # the cos / sin split at row 65 inside a tile; W = 130: a third DftAdj column tile of 2; depth
                    # 130 = 8 TK + 2; together with 4N = 68
    (129, 1, 5),    # M = 128, W = 256: every tile exact
    (131, 2, 3),    # M = 130: three row tiles with 2 rows in the last, exactly two from m = 2, exactly one from m = 66;
                    # LegAdj rows 131 and W = 260 ragged
]
SPIKE = 32.0
# Degree 0 has one real coefficient per field, so its coherence is 1 identically, and a low degree whose spike dominates
# both fields comes close: there the fp32 reference's 1 - coh is rounding noise, and its gradient is that noise over
# |c_pred|.  Among some hundred noise planes one or two have a |c_pred| at such a degree a few hundred times below the
# rms by chance, and the fp32 CPU evaluation of that plane is 1e-4 from fp64 (sht.hip sums the spectra in fp64 and is not
# affected).  The seed offset is one at which no plane of any case is in that corner; test_amse_cpu.py holds the fp32
# reference's own error of every case under a third of the ceiling, so a drifted recipe shows there and not on the GPU.
SEED = 50000


def edge_modes(H):
    """the (l, m) at the first and last row of each 64-row tile of an order's triangle and at the first, last and
    tile-edge orders: l in {0, 1, 63, 64, 65, M-2, M-1}, m in {0, 1, 63, 64, l-1, l}, where they exist"""
    M = H - 1
    return [(l, m) for l in sorted({0, 1, 63, 64, 65, M - 2, M - 1}) if 0 <= l < M
            for m in sorted({0, 1, 63, 64, l - 1, l}) if 0 <= m <= l]


def _tri_mask(H):
    """[H, H] bool: the coefficients AMSE reads (l < H - 1, m <= l)"""
    l = torch.arange(H).view(H, 1)
    m = torch.arange(H).view(1, H)
    return (l < H - 1) & (m <= l)


@functools.lru_cache(maxsize=None)
def edge_fields(H, B, C):
    """(pred, target) fp32 [B, C, H, 2(H-1)] of one tile-edge case (cached: read-only).  Target = white noise plus
    spectral spikes, pred = independent white noise plus half the same spikes.  Plane n carries a third of edge_modes(H),
    rotated by n, each at SPIKE times the rms coefficient magnitude of the noise (from the fp64 transform), so a dropped
    or doubled edge coefficient is visible; plane n is then scaled by 1 + n / N, so no two planes are alike.  The fields
    are dense, so both pole rows, the first and last longitude and the elements next to each depth-step boundary carry
    full weight already."""
    from _util import seeded
    W, N = 2 * (H - 1), B * C
    noise_t = seeded(SEED + 7 * H + N, N, H, W).double()
    noise_p = seeded(SEED + 7 * H + N + 5000, N, H, W).double()
    c = sht(noise_t)
    amp = SPIKE * float(c.abs().pow(2)[:, _tri_mask(H)].mean().sqrt())
    em = edge_modes(H)
    unit = []
    for e, (l, m) in enumerate(em):
        coef = amp * (-1.0) ** e if m == 0 else amp * complex(math.cos(0.5 + e), math.sin(0.5 + e))
        unit.append(synth(H, W, {(l, m): coef}))
    unit = torch.stack(unit).reshape(len(em), H * W)
    sel = torch.zeros(N, len(em), dtype=torch.float64)
    for n in range(N):
        for j in range((len(em) + 2) // 3):
            sel[n, (n + 3 * j) % len(em)] = 1.0
    spikes = (sel @ unit).view(N, H, W)
    s = (1.0 + torch.arange(N, dtype=torch.float64) / N).view(N, 1, 1)
    pred = ((noise_p + 0.5 * spikes) * s).float().view(B, C, H, W)
    target = ((noise_t + spikes) * s).float().view(B, C, H, W)
    return pred, target


def plane_err(g, g64):
    """max over the planes n of max|g_n - g64_n| / max|g64_n|"""
    d = (g.double() - g64).abs().amax((-2, -1))
    return float((d / g64.abs().amax((-2, -1)).clamp_min(1e-300)).max())


def errors(v, g, v64, g64):
    """{value, grad, plane}: relative error of the value, max_rel of the whole gradient, worst plane's max_rel"""
    d = (g.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-300)
    return {"value": abs(v - v64) / abs(v64), "grad": float(d), "plane": plane_err(g, g64)}


@functools.lru_cache(maxsize=None)
def edge_reference(H, B, C):
    """(v64, g64, e_cpu) of one tile-edge case (cached: read-only): the fp64 value and gradient, and the larger error
    of the two fp32 CPU evaluations (dft="fft" and dft="matrix") of the value, the whole gradient and the worst plane"""
    pred, target = edge_fields(H, B, C)
    v64, g64 = value_and_grad(pred, target, torch.float64)
    e32 = [errors(*value_and_grad(pred, target, torch.float32, dft), v64, g64) for dft in ("fft", "matrix")]
    return v64, g64, {k: max(e[k] for e in e32) for k in e32[0]}
