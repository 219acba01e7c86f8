"""Plain numpy restatement of ``paradis_model_amd.events`` (csrc/events.hip): values and decisions in ``np.float32``
operations in the order the module states, counts as integer sums, weights applied in float64.  Not a test module.

A source is a dict ``{"kind": "plain" | "speed" | "anomaly", "c0": int, "c1": int (speed only), "thresholds": [..],
"direction": "ge" | "le"}``.  ``counts`` also returns the number of AMBIGUOUS cells: cells whose fp64 value of ``x``
lies within 4 fp32 ulps of a threshold without being exactly equal to it in fp32 and in fp64 - cells where a different
(but still correct to the last bit or two) evaluation order could decide the other way.  A design whose count is zero
has one answer only.
"""
import numpy as np

F32 = np.float32


def values(v, kind, c0, c1, clim_rows):
    """(x [B, H, W] float32, x64 float64, valid bool) of one field ``v [B, C, H, W]`` float32; ``clim_rows``: [B, H, W]
    float32 climatology planes of channel c0 (anomaly; non-finite where the sample's slot is out of range)"""
    v = np.asarray(v, F32)
    a = v[:, c0]
    with np.errstate(all="ignore"):
        if kind == "plain":
            return a, a.astype(np.float64), np.isfinite(a)
        if kind == "speed":
            b = v[:, c1]
            x = np.sqrt((a * a + b * b).astype(F32)).astype(F32)          # mul, mul, add, sqrt: each rounded to fp32
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            return x, np.sqrt(a64 * a64 + b64 * b64), np.isfinite(a) & np.isfinite(b)
        if kind == "anomaly":
            x = (a - clim_rows).astype(F32)
            return x, a.astype(np.float64) - clim_rows.astype(np.float64), np.isfinite(a) & np.isfinite(clim_rows)
    raise ValueError(kind)


def counts(f, t, sources, clim=None, clim_index=None):
    """integer rows of ONE update: ``valid [S, H]``, ``forecast_yes``, ``observed_yes``, ``both [S, H, T]`` (int64; -1
    past a source's own thresholds) and ``ambiguous`` (int)"""
    f, t = np.asarray(f, F32), np.asarray(t, F32)
    B, C, H, W = f.shape
    S, T = len(sources), max(len(s["thresholds"]) for s in sources)
    out = {"valid": np.zeros((S, H), np.int64), "forecast_yes": np.full((S, H, T), -1, np.int64),
           "observed_yes": np.full((S, H, T), -1, np.int64), "both": np.full((S, H, T), -1, np.int64), "ambiguous": 0}
    for s, src in enumerate(sources):
        kind, c0, c1 = src["kind"], src["c0"], src.get("c1", 0)
        rows = None
        if kind == "anomaly":
            K = clim.shape[0]
            k = np.zeros(B, np.int64) if clim_index is None else np.asarray(clim_index, np.int64)
            rows = np.full((B, H, W), np.nan, F32)                         # a slot out of range: no valid cell
            for b in range(B):
                if 0 <= k[b] < K:
                    rows[b] = clim[k[b], c0]
        xf, xf64, vf = values(f, kind, c0, c1, rows)
        xt, xt64, vt = values(t, kind, c0, c1, rows)
        valid = vf & vt
        out["valid"][s] = valid.sum(axis=(0, 2))
        sign = F32(1.0 if src["direction"] == "ge" else -1.0)
        with np.errstate(all="ignore"):
            sf, st = (sign * xf).astype(F32), (sign * xt).astype(F32)
        for j, thr in enumerate(src["thresholds"]):
            thr32 = F32(thr)
            tp = F32(sign * thr32)
            with np.errstate(all="ignore"):
                F = valid & (sf >= tp)
                O = valid & (st >= tp)
            out["forecast_yes"][s, :, j] = F.sum(axis=(0, 2))
            out["observed_yes"][s, :, j] = O.sum(axis=(0, 2))
            out["both"][s, :, j] = (F & O).sum(axis=(0, 2))
            for x32, x64 in ((xf, xf64), (xt, xt64)):
                with np.errstate(all="ignore"):
                    ulp = np.spacing(np.maximum(np.abs(x32), np.abs(thr32)).astype(F32)).astype(np.float64)
                    near = valid & (np.abs(x64 - np.float64(thr32)) <= 4.0 * ulp)
                    tie = (x32 == thr32) & (x64 == np.float64(thr32))
                out["ambiguous"] += int((near & ~tie).sum())
    return out


def add_counts(total, one):
    """accumulates ``counts`` of several updates (``total`` None at first); -1 entries stay -1"""
    if total is None:
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in one.items()}
    for k in ("valid", "forecast_yes", "observed_yes", "both"):
        total[k] = np.where(one[k] < 0, -1, total[k] + one[k])
    total["ambiguous"] += one["ambiguous"]
    return total


def tables(cnt, band_w):
    """float64 ``(a, b, c, d)`` each ``[S, R, T]`` from integer rows ``[S, H(, T)]`` and band weights ``[R, H]``: the
    weighted rows are summed one by one, in row order; NaN past a source's thresholds"""
    nV, nF, nO, nFO = cnt["valid"], cnt["forecast_yes"], cnt["observed_yes"], cnt["both"]
    S, H, T = nF.shape
    R = band_w.shape[0]
    a, b, c, d = (np.zeros((S, R, T), np.float64) for _ in range(4))
    for s in range(S):
        for j in range(T):
            if nF[s, 0, j] < 0:
                for x in (a, b, c, d):
                    x[s, :, j] = np.nan
                continue
            for r in range(R):
                for h in range(H):
                    w = float(band_w[r, h])
                    a[s, r, j] += w * float(nFO[s, h, j])
                    b[s, r, j] += w * float(nF[s, h, j] - nFO[s, h, j])
                    c[s, r, j] += w * float(nO[s, h, j] - nFO[s, h, j])
                    d[s, r, j] += w * float(nV[s, h] - nF[s, h, j] - nO[s, h, j] + nFO[s, h, j])
    return a, b, c, d
