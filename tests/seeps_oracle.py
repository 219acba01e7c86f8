"""Plain numpy restatement of SEEPS (paradis_model_amd/climatology.py ``build_seeps``, paradis_model_amd/seeps.py,
csrc/quantile.hip's SEEPS stage, csrc/seeps.hip), for the tests: Python loops over cells and Python doubles (IEEE divide,
multiply, add, subtract, floor; one rounding to float32 where the definition rounds).  It holds the climatology, the
per-row accumulators and the report.  The slot lists are ``clim_oracle.slot_lists`` / ``clim_oracle.csr``.  The
definitions are the project's own restatement of Rodwell et al. (2010); nothing here is pinned against a package.  Test
infrastructure; reads nothing outside the repository."""
import math

import numpy as np

from tests import clim_oracle as CO

slot_lists, csr = CO.slot_lists, CO.csr

NAN32 = np.float32(np.nan)


# ---------------------------------------------------------------------------------- the climatology
def cell_climatology(values, dry, wet_level=2.0 / 3.0, min_count=1):
    """one cell: ``values`` any float array, ``dry`` a float32 -> ``(p1, thr)`` as np.float32"""
    dry = float(np.float32(dry))
    v = np.asarray(values, np.float64).reshape(-1)
    v = np.sort(v[np.isfinite(v)] + 0.0)              # -0.0 + 0.0 == +0.0: read as +0.0
    m = int(v.size)
    if m < max(int(min_count), 1):
        return NAN32, NAN32
    n_dry = 0
    for x in v.tolist():
        if x < dry:                                   # strict; (-0.0 as a threshold compares as +0.0 does)
            n_dry += 1
    n_wet = m - n_dry
    p1 = np.float32(float(n_dry) / float(m))
    if n_wet < 1:
        return p1, NAN32
    pos = float(wet_level) * float(n_wet - 1)
    lo = math.floor(pos)
    hi = min(lo + 1, n_wet - 1)
    frac = pos - float(lo)
    a, b = float(v[n_dry + lo]), float(v[n_dry + hi])
    return p1, np.float32(a + (b - a) * frac)


def slot_climatology(x, lists, cols, dry, wet_level=2.0 / 3.0, min_count=1):
    """x [T, F, H, W] float32 numpy; ``lists``: per slot a list of rows (or of (row, weight) pairs, the weight is not
    read) -> float32 [2, K, C, H, W]: plane 0 p1, plane 1 thr"""
    T, F, H, W = x.shape
    out = np.full((2, len(lists), len(cols), H, W), np.nan, np.float32)
    for k, entries in enumerate(lists):
        rows = [int(e[0]) if isinstance(e, tuple) else int(e) for e in entries]
        if not rows:
            continue
        for c, col in enumerate(cols):
            block = x[rows, col].astype(np.float64)                     # [n, H, W]
            for h in range(H):
                for w in range(W):
                    out[:, k, c, h, w] = cell_climatology(block[:, h, w], dry, wet_level, min_count)
    return out


def classes(data, p_lo=0.1, p_hi=0.85):
    """the cells of a climatology ``[2, ...]`` by class: bool arrays ``below`` (p1 < p_lo), ``inside``, ``above``
    (p1 > p_hi; an all-dry cell is one of these too) and ``all_dry`` (p1 finite, thr NaN); ``inside`` asks for a finite
    thr as well: the cells that can be valid"""
    p1, thr = np.asarray(data[0], np.float32), np.asarray(data[1], np.float32)
    lo, hi = np.float32(p_lo), np.float32(p_hi)
    fin = np.isfinite(p1)
    with np.errstate(invalid="ignore"):
        return {"below": fin & (p1 < lo), "inside": fin & np.isfinite(thr) & (p1 >= lo) & (p1 <= hi),
                "above": fin & (p1 > hi), "all_dry": fin & np.isnan(thr)}


# ---------------------------------------------------------------------------------- the score
def matrix(p):
    """the 3x3 scoring matrix for the Python double ``p``: row the forecast category, column the truth category"""
    a = 1.0 / (1.0 - p)
    b = 1.0 / p
    c = 3.0 / (2.0 + p)
    return [[0.0, a, 4.0 * a], [b, 0.0, 3.0 * a], [b + c, c, 0.0]]


def category(x, dry, thr):
    """0 dry, 1 light, 2 heavy: comparisons of float32 values"""
    x, dry, thr = np.float32(x), np.float32(dry), np.float32(thr)
    if x < dry:
        return 0
    return 2 if x >= thr else 1


def cell_score(f, o, p1, thr, dry, p_lo, p_hi, slot_ok=True):
    """one cell -> ``("valid", cf, co, s)``, ``("masked",)`` or ``("none",)``; ``s`` a Python double"""
    vals = [np.float32(v) for v in (f, o, p1, thr)]
    if not slot_ok or not all(np.isfinite(v) for v in vals):
        return ("none",)
    p1 = vals[2]
    if not (np.float32(p_lo) <= p1 <= np.float32(p_hi)):
        return ("masked",)
    cf, co = category(f, dry, thr), category(o, dry, thr)
    return ("valid", cf, co, 0.5 * matrix(float(p1))[cf][co])


def rows(fc, truth, data, clim_index, chan, dry, p_lo=0.1, p_hi=0.85):
    """fc / truth [B, C, H, W] float32, data [2, K, Cs, H, W], clim_index [B], chan [Cs] state channels -> ``(real
    [Cs, H, 3] float64, ints [Cs, H, 10] int64, cells)``: the row sums (added cell by cell, b then w ascending) and the
    counters ``{n[cf][co] (cf-major), n_masked}``; ``cells[(cs, h)]``: the list of ``(b, w, cf, co, s)`` of the row's
    valid cells"""
    B, C, H, W = fc.shape
    K, Cs = data.shape[1], data.shape[2]
    real = np.zeros((Cs, H, 3), np.float64)
    ints = np.zeros((Cs, H, 10), np.int64)
    cells = {}
    for cs in range(Cs):
        c = int(chan[cs])
        for h in range(H):
            sums, here = [0.0, 0.0, 0.0], []
            for b in range(B):
                k = int(clim_index[b])
                if not 0 <= k < K:
                    continue
                for w in range(W):
                    r = cell_score(fc[b, c, h, w], truth[b, c, h, w], data[0, k, cs, h, w], data[1, k, cs, h, w], dry,
                                   p_lo, p_hi)
                    if r[0] == "masked":
                        ints[cs, h, 9] += 1
                    elif r[0] == "valid":
                        _, cf, co, s = r
                        ints[cs, h, 3 * cf + co] += 1
                        sums[co] += s
                        here.append((b, w, cf, co, s))
            real[cs, h] = sums
            cells[(cs, h)] = here
    return real, ints, cells


def report(real, ints, n, band_w):
    """real [L, Cs, H, 3], ints [L, Cs, H, 10], n [L], band_w [R, H] -> dict of float64 arrays as
    ``seeps.report`` gives them, by plain loops"""
    L, Cs, H, _ = real.shape
    R = band_w.shape[0]
    nan = float("nan")
    out = {"seeps": np.full((L, Cs, R), nan), "seeps_skill": np.full((L, Cs, R), nan),
           "coverage": np.full((L, Cs, R), nan), "by_truth": np.full((L, Cs, R, 3), nan),
           "categories": np.full((L, Cs, R, 3, 3), nan), "forecast_freq": np.full((L, Cs, R, 3), nan),
           "truth_freq": np.full((L, Cs, R, 3), nan)}
    for l in range(L):
        if int(n[l]) == 0:
            continue
        for c in range(Cs):
            for r in range(R):
                N, S, cat, masked = 0.0, [0.0, 0.0, 0.0], [0.0] * 9, 0.0
                for h in range(H):
                    w = float(band_w[r, h])
                    N += w * float(sum(int(v) for v in ints[l, c, h, :9]))
                    masked += w * float(ints[l, c, h, 9])
                    for j in range(3):
                        S[j] += w * float(real[l, c, h, j])
                    for j in range(9):
                        cat[j] += w * float(ints[l, c, h, j])
                if N + masked != 0.0:
                    out["coverage"][l, c, r] = N / (N + masked)
                if N == 0.0:
                    continue
                seeps = ((S[0] + S[1]) + S[2]) / N
                out["seeps"][l, c, r] = seeps
                out["seeps_skill"][l, c, r] = 1.0 - seeps
                out["by_truth"][l, c, r] = [s / N for s in S]
                freq = np.array(cat).reshape(3, 3) / N
                out["categories"][l, c, r] = freq
                out["forecast_freq"][l, c, r] = freq.sum(axis=1)
                out["truth_freq"][l, c, r] = freq.sum(axis=0)
    return out
