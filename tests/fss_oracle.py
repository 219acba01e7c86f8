"""Plain numpy restatement of ``paradis_model_amd.neighbourhood`` (csrc/fss.hip): the event decision is
``tests/events_oracle.py``'s (values and comparisons in ``np.float32``), everything after it is int64.  Not a test module.

A source is the dict of ``events_oracle``.  ``scales``: latitude half-widths ``ny[k]``; ``half_x``: int ``[K, H]``
longitude half-widths per centre row.  The window of centre cell ``(h, w)`` is rows ``max(0, h - ny) .. min(H - 1,
h + ny)`` and columns ``w - nx[k][h] .. w + nx[k][h]`` modulo ``W`` (``2 nx + 1 <= W``: no cell is met twice).

Two versions of the window sums: ``window_sums_brute`` visits the cells of every window one by one;
``window_sums_fast`` adds clipped column sums and rolls them along the longitude.  ``counts`` takes either.
"""
import numpy as np

from tests import events_oracle as EO

F32 = np.float32


def event_bits(f, t, sources, clim=None, clim_index=None):
    """per source ``(F, O [B, n, H, W] bool, valid [B, H, W] bool)``: an invalid cell is a non-event in both fields"""
    f, t = np.asarray(f, F32), np.asarray(t, F32)
    B, C, H, W = f.shape
    out = []
    for src in sources:
        kind, c0, c1 = src["kind"], src["c0"], src.get("c1", 0)
        rows = None
        if kind == "anomaly":
            K = clim.shape[0]
            k = np.zeros(B, np.int64) if clim_index is None else np.asarray(clim_index, np.int64)
            rows = np.full((B, H, W), np.nan, F32)                         # a slot out of range: no valid cell
            for b in range(B):
                if 0 <= k[b] < K:
                    rows[b] = clim[k[b], c0]
        xf, _, vf = EO.values(f, kind, c0, c1, rows)
        xt, _, vt = EO.values(t, kind, c0, c1, rows)
        valid = vf & vt
        sign = F32(1.0 if src["direction"] == "ge" else -1.0)
        with np.errstate(all="ignore"):
            sf, st = (sign * xf).astype(F32), (sign * xt).astype(F32)
            thr = [F32(sign * F32(v)) for v in src["thresholds"]]
            F = np.stack([valid & (sf >= v) for v in thr], axis=1)
            O = np.stack([valid & (st >= v) for v in thr], axis=1)
        out.append((F, O, valid))
    return out


def window_sums_brute(F, O, ny, nx):
    """``(FF, OO, FO) [H, n]`` int64 of bits ``F, O [B, n, H, W]``, half-width ``ny`` and ``nx [H]``: loops over the
    centre cells and over the cells of each window"""
    B, n, H, W = F.shape
    Fi, Oi = F.astype(np.int64), O.astype(np.int64)
    FF, OO, FO = (np.zeros((H, n), np.int64) for _ in range(3))
    for h in range(H):
        for w in range(W):
            cF, cO = np.zeros((B, n), np.int64), np.zeros((B, n), np.int64)
            for y in range(h - ny, h + ny + 1):
                if y < 0 or y > H - 1:
                    continue
                for x in range(w - int(nx[h]), w + int(nx[h]) + 1):
                    cF += Fi[:, :, y, x % W]
                    cO += Oi[:, :, y, x % W]
            FF[h] += (cF * cF).sum(axis=0)
            OO[h] += (cO * cO).sum(axis=0)
            FO[h] += (cF * cO).sum(axis=0)
    return FF, OO, FO


def window_sums_fast(F, O, ny, nx):
    """the same sums from clipped column sums (a cumulative sum along the latitude) and ``np.roll`` along the longitude"""
    B, n, H, W = F.shape
    out = []
    counts = []
    for X in (F, O):
        cs = np.concatenate([np.zeros((B, n, 1, W), np.int64), np.cumsum(X.astype(np.int64), axis=2)], axis=2)
        lo = np.maximum(0, np.arange(H) - ny)
        hi = np.minimum(H - 1, np.arange(H) + ny) + 1
        col = cs[:, :, hi] - cs[:, :, lo]                                   # [B, n, H, W] vertical counts
        c = np.zeros_like(col)
        for h in range(H):
            for d in range(-int(nx[h]), int(nx[h]) + 1):
                c[:, :, h] += np.roll(col[:, :, h], d, axis=-1)
        counts.append(c)
    cF, cO = counts
    out = ((cF * cF).sum(axis=(0, 3)).T, (cO * cO).sum(axis=(0, 3)).T, (cF * cO).sum(axis=(0, 3)).T)
    return tuple(np.ascontiguousarray(x) for x in out)


def counts(f, t, sources, scales, half_x, clim=None, clim_index=None, window_sums=window_sums_fast):
    """int64 arrays of ONE update: ``valid [S, H]``, ``forecast_yes``, ``observed_yes [S, H, T]``, ``ff``, ``oo``, ``fo``
    ``[S, H, K, T]`` (-1 past a source's own thresholds)"""
    half_x = np.asarray(half_x)
    S, K, T = len(sources), len(scales), max(len(s["thresholds"]) for s in sources)
    H = np.asarray(f).shape[2]
    assert half_x.shape == (K, H)
    out = {"valid": np.zeros((S, H), np.int64), "forecast_yes": np.full((S, H, T), -1, np.int64),
           "observed_yes": np.full((S, H, T), -1, np.int64), "ff": np.full((S, H, K, T), -1, np.int64),
           "oo": np.full((S, H, K, T), -1, np.int64), "fo": np.full((S, H, K, T), -1, np.int64)}
    for s, (F, O, valid) in enumerate(event_bits(f, t, sources, clim, clim_index)):
        n = F.shape[1]
        out["valid"][s] = valid.sum(axis=(0, 2))
        out["forecast_yes"][s, :, :n] = F.sum(axis=(0, 3)).T
        out["observed_yes"][s, :, :n] = O.sum(axis=(0, 3)).T
        for k, ny in enumerate(scales):
            FF, OO, FO = window_sums(F, O, int(ny), half_x[k])
            out["ff"][s, :, k, :n], out["oo"][s, :, k, :n], out["fo"][s, :, k, :n] = FF, OO, FO
    return out


KEYS = ("valid", "forecast_yes", "observed_yes", "ff", "oo", "fo")


def add_counts(total, one):
    """accumulates ``counts`` of several updates (``total`` None at first); -1 entries stay -1"""
    if total is None:
        return {k: v.copy() for k, v in one.items()}
    for k in KEYS:
        total[k] = np.where(one[k] < 0, -1, total[k] + one[k])
    return total
