"""Plain numpy restatement of the quantile climatology (paradis_model_amd/climatology.py ``build_quantiles``,
csrc/quantile.hip), for the tests: a Python loop over cells, ``np.sort`` of the finite values as float64 and the stated
formula in Python doubles (IEEE multiply, subtract, add, floor; one rounding to float32).  The slot lists are
``clim_oracle.slot_lists`` / ``clim_oracle.csr``.  Test infrastructure; reads nothing outside the repository."""
import math

import numpy as np

from tests import clim_oracle as CO

slot_lists, csr = CO.slot_lists, CO.csr


def cell_quantiles(values, levels, min_count=1):
    """one cell: ``values`` any float array, ``levels`` Python floats in [0, 1] -> list of np.float32"""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[np.isfinite(v)] + 0.0                       # -0.0 + 0.0 == +0.0: read as +0.0
    m = int(v.size)
    if m < max(int(min_count), 1):
        return [np.float32(np.nan)] * len(levels)
    v = np.sort(v)
    out = []
    for q in levels:
        pos = float(q) * float(m - 1)
        lo = math.floor(pos)
        hi = min(lo + 1, m - 1)
        frac = pos - float(lo)
        a, b = float(v[lo]), float(v[hi])
        out.append(np.float32(a + (b - a) * frac))
    return out


def slot_quantiles(x, lists, cols, levels, min_count=1):
    """x [T, F, H, W] float32 numpy; ``lists``: per slot a list of rows (or of (row, weight) pairs, the weight is not
    read) -> float32 [Q, K, C, H, W]"""
    T, F, H, W = x.shape
    levels = [float(q) for q in levels]
    out = np.full((len(levels), len(lists), len(cols), H, W), np.nan, np.float32)
    for k, entries in enumerate(lists):
        rows = [int(e[0]) if isinstance(e, tuple) else int(e) for e in entries]
        if not rows:
            continue
        for c, col in enumerate(cols):
            block = x[rows, col].astype(np.float64)                     # [n, H, W]
            for h in range(H):
                for w in range(W):
                    out[:, k, c, h, w] = cell_quantiles(block[:, h, w], levels, min_count)
    return out
