"""Forecast verification scores in plain torch: a restatement of the conventions of ``paradis_model_amd/verify.py``
(WeatherBench-2's deterministic scores) that imports nothing from the package.

Forecast ``f`` and truth ``t`` ``[B, C, H, W]``, latitude weights ``w [H] >= 0``, ``Z = W * sum_h w[h]`` (double),
optional climatology ``clim [K, C, H, W]`` with the slot ``k[b]`` of every sample.  Per sample and channel, sums over
the plane, ``fa = f - clim[k[b]]``, ``ta = t - clim[k[b]]``::

    se = sum w (f-t)^2 / Z      e  = sum w (f-t) / Z      ae = sum w |f-t| / Z
    ff = sum w fa^2             tt = sum w ta^2            ft = sum w fa ta
    acc_b = ft / sqrt(ff * tt)       (the sample is left out of the ACC mean when ff * tt == 0)

accumulated per (lead, channel) as ``{n, sum se, sum e, sum ae, sum acc_b, n_acc, sum ff, sum tt}`` and reported as
``rmse = sqrt(sum se / n)``, ``bias = sum e / n``, ``mae = sum ae / n``, ``acc = sum acc_b / n_acc``,
``activity = sqrt(sum ff / sum tt)``, ``count = n``.

``dtype=torch.float64`` is the reference.  ``dtype=torch.float32`` is the yardstick of the GPU tests: the same
element-wise formulas and the plane sums in float32 ATen on the CPU (``seq=True``: a strictly sequential float32 sum, as
``tests/test_hip_kernel_edges.py::_seq_sum``); what follows the plane sums is double either way, as the accumulators are.
"""
import numpy as np
import torch

METRICS = ("rmse", "bias", "mae", "acc", "activity")
FIELDS = 8


def _seq_sum(terms):
    """strictly sequential fp32 sum over the last axis of an fp32 CPU tensor"""
    a = np.ascontiguousarray(terms.detach().cpu().numpy().astype(np.float32, copy=False))
    return torch.from_numpy(np.cumsum(a, axis=-1, dtype=np.float32)[..., -1].copy())


def normaliser(w, W):
    return float(W) * float(torch.as_tensor(w).detach().double().sum())


def plane_sums(f, t, w, clim=None, k=None, dtype=torch.float64, seq=False):
    """the weighted sums of every plane, as double ``[B, C]`` tensors: s0 .. s2 (and s3 .. s5 with a climatology) =
    sum w (f-t)^2, sum w (f-t), sum w |f-t|, sum w fa^2, sum w ta^2, sum w fa ta; not yet divided by Z"""
    f, t = f.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    B, C, H, W = f.shape
    wv = torch.as_tensor(w).detach().cpu().to(dtype).reshape(1, 1, H, 1)

    def tot(x):
        x = x.reshape(B, C, H * W)
        return (_seq_sum(x) if seq else x.sum(-1)).double()

    d = f - t
    sums = [tot(wv * (d * d)), tot(wv * d), tot(wv * d.abs())]
    if clim is not None:
        cl = clim.detach().cpu().to(dtype)[torch.as_tensor(k).detach().cpu().long()]
        fa, ta = f - cl, t - cl
        sums += [tot(wv * (fa * fa)), tot(wv * (ta * ta)), tot(wv * (fa * ta))]
    return sums


def accumulate(acc, sums, Z):
    """adds the samples of one ``plane_sums`` result, in batch order, to ``acc`` (double ``[C, 8]``, in place)"""
    B = sums[0].shape[0]
    for b in range(B):
        acc[:, 0] += 1.0
        acc[:, 1] += sums[0][b] / Z
        acc[:, 2] += sums[1][b] / Z
        acc[:, 3] += sums[2][b] / Z
        if len(sums) > 3:
            ff, tt, ft = sums[3][b], sums[4][b], sums[5][b]
            keep = (ff * tt) != 0
            acc[:, 4] += torch.where(keep, ft / torch.sqrt(torch.where(keep, ff * tt, torch.ones_like(ff))),
                                     torch.zeros_like(ff))
            acc[:, 5] += keep.double()
            acc[:, 6] += ff
            acc[:, 7] += tt
    return acc


def report(acc, with_clim):
    """``acc`` double ``[n_leads, C, 8]`` -> the reported values: float64 numpy ``[n_leads, C]`` per metric, ``count``
    ``[n_leads]``; NaN where a lead was never updated, and for acc / activity without a climatology"""
    a = acc.detach().cpu().double().numpy()
    n = a[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"rmse": np.sqrt(a[..., 1] / n), "bias": a[..., 2] / n, "mae": a[..., 3] / n,
               "acc": a[..., 4] / a[..., 5] if with_clim else np.full(n.shape, np.nan),
               "activity": np.sqrt(a[..., 6] / a[..., 7]) if with_clim else np.full(n.shape, np.nan)}
    for key in METRICS:
        res[key] = np.where(n > 0, res[key], np.nan)
    res["count"] = n[:, 0].copy()
    return res


def scores(updates, w, n_leads, C, clim=None, dtype=torch.float64, seq=False):
    """``updates``: a list of ``(lead, f, t, k or None)`` -> ``(acc [n_leads, C, 8], report(acc))``"""
    acc = torch.zeros(n_leads, C, FIELDS, dtype=torch.float64)
    for lead, f, t, k in updates:
        if f.shape[0] == 0:
            continue
        use = clim if clim is not None else None
        if use is not None and k is None:
            k = torch.zeros(f.shape[0], dtype=torch.long)
        accumulate(acc[lead], plane_sums(f, t, w, use, k, dtype, seq), normaliser(w, f.shape[-1]))
    return acc, report(acc, clim is not None)
