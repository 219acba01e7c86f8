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
"""
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


def dense_weights(nlat, nlon):
    """torch_harmonics' dense layout [mmax, lmax, nlat] (lmax = nlat, mmax = nlon//2 + 1), fp64"""
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

    def forward(self, x):
        assert x.shape[-2] == self.nlat and x.shape[-1] == self.nlon
        x = 2.0 * torch.pi * torch.fft.rfft(x, dim=-1, norm="forward")
        x = torch.view_as_real(x[..., : self.mmax])
        w = self.weights.to(x.dtype)
        re = torch.einsum("...km,mlk->...lm", x[..., 0], w)
        im = torch.einsum("...km,mlk->...lm", x[..., 1], w)
        return torch.complex(re, im)


def sht(x, dtype=torch.float64):
    """coefficients [..., nlat, nlon//2+1] of x in `dtype` arithmetic (fp64: the accuracy yardstick)"""
    m = RealSHT(x.shape[-2], x.shape[-1])
    if dtype == torch.float64:
        m.weights = dense_weights(x.shape[-2], x.shape[-1])
    return m(x.to(dtype))


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


def amse(pred, target, dtype=torch.float64):
    """scalar AMSE (unweighted); NaN -> 1e6 as the reference"""
    loss = amse_from_coeffs(sht(pred, dtype), sht(target.detach(), dtype))
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
