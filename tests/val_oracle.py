"""CPU restatement of the validation scores, written from the formulas, for the tests: the row
``[1 + 2C + R]`` = (validation loss, per-channel loss weighted / unweighted, report RMSE in physical units) of one step
in plain fp64 or in fp32 in the reference's operation order (utils/loss.py:105-127,233-282, trainer.py:291-315,
utils/normalization.py:39-52,69-80), and the seeded inputs the golden generator uses.  Checked against the reference's
own numbers (tests/golden/v1_val.pt) by tests/test_val_cpu.py."""
import numpy as np
import torch

from tests import forecast_oracle as FO

CLS_Z, CLS_HUM, CLS_PRECIP = 1, 2, 3          # codes of paradis_normalize_features
BRANCH = {"zscore": CLS_Z, "humidity": CLS_HUM, "precipitation": CLS_PRECIP}
SINGLE_REPORTS = ["geopotential_h500", "specific_humidity_h850", "total_precipitation_6hr", "2m_temperature",
                  "geopotential_h500"]
ROLLOUT_REPORTS = ["geopotential_h500", "specific_humidity_h850", "2m_temperature"]


def report_std(names, report_features, seed=501):
    """the std of each report feature: FO.channel_stats at the feature's channel (what a dataset's report_stats hold)"""
    _, std = FO.channel_stats(names, seed)
    return torch.stack([std[names.index(f)] for f in report_features]) if report_features else torch.zeros(0)


def single_state(seed, names, B, H, W):
    """(pred, target) [B, C, H, W]: a seeded normalised target (humidity / precipitation channels in their ranges) and
    pred = target + 0.3 randn"""
    C = len(names)
    target = FO.normalised_state(seed, names, B, C, H, W)
    g = torch.Generator().manual_seed(seed + 1000)
    return target + 0.3 * torch.randn(B, C, H, W, generator=g), target


def loss_term(e, kind, delta):
    if kind == "mse":
        return e ** 2
    a = e.abs()
    s = 1 / (1 + torch.exp(-2 * (a - delta)))
    return (1 - s) * (delta * a) + s * ((e ** 2 + delta ** 2) / (2 * delta))


def denorm(x, cls, p0, p1):
    """x in its own dtype; p0 / p1 fp32 table values (q_min, q_max), widened when x is fp64"""
    if cls == CLS_HUM:
        qmin, qmax = torch.tensor(p0, dtype=torch.float32).to(x.dtype), torch.tensor(p1, dtype=torch.float32).to(x.dtype)
        q = torch.exp(x * (torch.log(qmax) - torch.log(qmin)) + torch.log(qmin)) - 1e-12
        return torch.clip(q, min=0, max=float(qmax))
    if cls == CLS_PRECIP:
        return torch.clip(torch.exp(x - 10) - 1e-6, min=0)
    raise ValueError(cls)


def _mean(t, dims, seq):
    """mean over ``dims``; ``seq``: a strictly sequential fp32 sum (numpy.cumsum) divided in fp32"""
    if not seq:
        return t.mean(dim=dims) if dims is not None else t.mean()
    a = t.detach().numpy().astype(np.float32, copy=False)
    if dims is None:
        flat, n = a.reshape(1, -1), a.size
    else:
        keep = [d for d in range(a.ndim) if d not in dims]
        flat = np.ascontiguousarray(np.transpose(a, keep + list(dims))).reshape(int(np.prod([a.shape[d] for d in keep])), -1)
        n = flat.shape[1]
    s = np.cumsum(flat, axis=-1, dtype=np.float32)[..., -1] / np.float32(n)
    return torch.from_numpy(np.asarray(s).copy()).reshape(()) if dims is None else torch.from_numpy(s.copy())


def row(pred, target, wf, wl, lat_w, kind, delta, reports, dtype=torch.float64, seq=False):
    """[1 + 2C + R].  pred, target [B, C, H, W]; wf [C]; wl [H] or None (the loss's latitude weights when it applies
    them); lat_w [H] (reports); kind "mse" | "reversed_huber" | "none"; reports: list of (channel, class, p0, p1).
    ``dtype=torch.float32`` evaluates in the reference's operation order; ``seq`` sums sequentially (fp32 only)."""
    p, t = pred.detach().to(dtype), target.detach().to(dtype)
    C = p.shape[1]
    if kind == "none":
        head = torch.zeros(1 + 2 * C, dtype=dtype)
    else:
        l = loss_term(p - t, kind, delta)
        w = l * wf.to(dtype).view(1, -1, 1, 1)
        if wl is not None:
            w = w * wl.to(dtype).view(1, 1, -1, 1)
        head = torch.cat([_mean(w, None, seq).reshape(1), _mean(w, (0, 2, 3), seq), _mean(l, (0, 2, 3), seq)]).to(dtype)
    tail = []
    for (c, cls, p0, p1) in reports:
        lw = lat_w.to(dtype).view(1, -1, 1)
        if cls == CLS_Z:
            d = (t[:, c] - p[:, c]) * torch.tensor(p1, dtype=torch.float32).to(dtype)
        else:
            d = denorm(t[:, c], cls, p0, p1) - denorm(p[:, c], cls, p0, p1)
        tail.append(torch.sqrt(_mean(d ** 2 * lw, None, seq).to(dtype)).reshape(1))
    return torch.cat([head] + tail)


def report_tuples(names, report_features, custom, std):
    """(channel, class, p0, p1) per report feature, by the reference's branch order (trainer.py:297-313)"""
    out = []
    for r, f in enumerate(report_features):
        c = names.index(f)
        if custom and "specific_humidity" in f:
            out.append((c, CLS_HUM, FO.Q_MIN, FO.Q_MAX))
        elif custom and "precipitation" in f:
            out.append((c, CLS_PRECIP, 0.0, 1.0))
        else:
            out.append((c, CLS_Z, 0.0, float(std[r])))
    return out
