"""Plain numpy restatement of the probabilistic event verification (paradis_model_amd/probability.py,
csrc/probability.hip); imports nothing from the package.  Not a test module.

A source is a dict ``{"kind": "plain" | "speed" | "anomaly", "c0": int, "c1": int (speed only), "thresholds": [..],
"direction": "ge" | "le"}`` (tests/events_oracle.py's).  ``source_value`` forms the value of a source in ``np.float32``
operations in csrc/event_source.h's order (numpy's float32 arithmetic is IEEE single, one rounding per operation, never
contracted); ``joint_rows`` counts, per source, latitude row and threshold, the valid cells by (truth event ``o``,
members with the event ``k``) - the accumulators of one update; ``report`` is the host arithmetic with bands and
weights in float64, row by row; ``mann_whitney`` the ROC area from raw per-cell probabilities; ``quantile_thresholds``
the thresholds the tests' designs use."""
import numpy as np

F32 = np.float32
SCORES = ("brier", "brier_fair", "base_rate", "uncertainty", "reliability", "resolution", "bss", "roc_area")
CURVES = ("observed_frequency", "forecast_frequency", "pod", "pofd")


def source_value(v, kind, c0, c1, clim_rows):
    """``(x float32, valid bool)``, each ``[B, H, W]``, of one field ``v [B, C, H, W]`` float32; ``clim_rows``:
    ``[B, H, W]`` float32 climatology planes of channel c0 for an anomaly (validity of the climatology cell itself is the
    caller's: ``joint_rows`` folds it in once)"""
    v = np.asarray(v, F32)
    a = v[:, c0]
    with np.errstate(all="ignore"):
        if kind == "plain":
            return a, np.isfinite(a)
        if kind == "speed":
            b = v[:, c1]
            aa, bb = (a * a).astype(F32), (b * b).astype(F32)
            return np.sqrt((aa + bb).astype(F32)).astype(F32), np.isfinite(a) & np.isfinite(b)   # mul, mul, add, sqrt
        if kind == "anomaly":
            return (a - clim_rows).astype(F32), np.isfinite(a)
    raise ValueError(kind)


def clim_planes(src, clim, clim_index, G, H, W):
    """``[G, H, W]`` float32: the climatology plane of each ensemble for an anomaly source (NaN where the ensemble's slot
    is out of range: no valid cell), None for the other kinds"""
    if src["kind"] != "anomaly":
        return None
    K = clim.shape[0]
    k = np.zeros(G, np.int64) if clim_index is None else np.asarray(clim_index, np.int64)
    rows = np.full((G, H, W), np.nan, F32)
    for g in range(G):
        if 0 <= k[g] < K:
            rows[g] = clim[k[g], src["c0"]]
    return rows


def cell_counts(fc, truth, M, src, clim=None, clim_index=None):
    """per cell of one source: ``valid [G, H, W]`` bool, ``o [nthr, G, H, W]`` (0 / 1) and ``k [nthr, G, H, W]``
    (0 .. M), int64, and the truth's value ``x [G, H, W]`` float32"""
    fc, truth = np.asarray(fc, F32), np.asarray(truth, F32)
    GM, C, H, W = fc.shape
    G = GM // M
    assert G * M == GM and truth.shape == (G, C, H, W)
    kind, c0, c1 = src["kind"], src["c0"], src.get("c1", 0)
    rows = clim_planes(src, clim, clim_index, G, H, W)
    sign = F32(1.0 if src["direction"] == "ge" else -1.0)
    xt, valid = source_value(truth, kind, c0, c1, rows)
    if rows is not None:
        valid = valid & np.isfinite(rows)
    with np.errstate(all="ignore"):
        st = (sign * xt).astype(F32)
    nthr = len(src["thresholds"])
    tp = [F32(sign * F32(t)) for t in src["thresholds"]]              # thr' = sign * thr (exact)
    o = np.zeros((nthr, G, H, W), np.int64)
    k = np.zeros((nthr, G, H, W), np.int64)
    with np.errstate(all="ignore"):
        for j in range(nthr):
            o[j] = st >= tp[j]
        for i in range(M):
            xm, vm = source_value(fc[i::M], kind, c0, c1, rows)       # member i of every ensemble
            valid = valid & vm
            sm = (sign * xm).astype(F32)
            for j in range(nthr):
                k[j] += sm >= tp[j]
    return valid, o, k, xt


def joint_rows(fc, truth, M, sources, clim=None, clim_index=None):
    """one update: ``fc [G * M, C, H, W]`` member-minor, ``truth [G, C, H, W]`` -> ``(acc [S, H, 1 + T 2 (M + 1)] int64,
    detail)``: the accumulator row layout of the kernel, ``{nV, joint[T][2][M + 1]}`` with zeros past a source's own
    thresholds; ``detail[s] = (valid, o, k, x_truth)`` of ``cell_counts``"""
    H = fc.shape[2]
    S, T = len(sources), max(len(s["thresholds"]) for s in sources)
    acc = np.zeros((S, H, 1 + T * 2 * (M + 1)), np.int64)
    detail = []
    for s, src in enumerate(sources):
        valid, o, k, xt = cell_counts(fc, truth, M, src, clim, clim_index)
        acc[s, :, 0] = valid.sum(axis=(0, 2))
        for j in range(len(src["thresholds"])):
            bins = o[j] * (M + 1) + k[j]
            for h in range(H):
                row = np.bincount(bins[:, h][valid[:, h]], minlength=2 * (M + 1))
                acc[s, h, 1 + j * 2 * (M + 1):1 + (j + 1) * 2 * (M + 1)] = row
        detail.append((valid, o, k, xt))
    return acc, detail


def split(acc, M):
    """``(nV [..., H], joint [..., H, T, 2, M + 1])`` of accumulator rows"""
    T = (acc.shape[-1] - 1) // (2 * (M + 1))
    return acc[..., 0], acc[..., 1:].reshape(acc.shape[:-1] + (T, 2, M + 1))


def scores_of(N0, N1, M):
    """the scores and curves of ONE pair of weighted count vectors ``N0[k]``, ``N1[k]`` (plain Python floats, one bin
    after the other); a zero denominator gives NaN"""
    nan = float("nan")
    N0, N1 = [float(v) for v in N0], [float(v) for v in N1]
    n0, n1 = sum(N0), sum(N1)
    N = n0 + n1
    div = lambda a, b: a / b if b != 0 else nan                           # noqa: E731
    obar = div(n1, N)
    brier = fair = rel = res = 0.0
    for k in range(M + 1):
        p, Nk = k / M, N0[k] + N1[k]
        brier += N1[k] * (p - 1.0) ** 2 + N0[k] * p ** 2
        fair += Nk * k * (M - k)
        if Nk > 0:
            rel += Nk * (p - N1[k] / Nk) ** 2
            res += Nk * (N1[k] / Nk - obar) ** 2
    brier, rel, res = div(brier, N), div(rel, N), div(res, N)
    unc = obar * (1.0 - obar)
    pod = [div(sum(N1[q:]), n1) for q in range(M + 2)]                    # q = M + 1: (0, 0)
    pofd = [div(sum(N0[q:]), n0) for q in range(M + 2)]
    roc = sum((pofd[q] - pofd[q + 1]) * (pod[q] + pod[q + 1]) / 2.0 for q in range(M + 1))
    return {"brier": brier, "brier_fair": brier - div(fair, M * M * (M - 1) * N), "base_rate": obar, "uncertainty": unc,
            "reliability": rel, "resolution": res, "bss": 1.0 - div(brier, unc), "roc_area": roc,
            "observed_frequency": [div(N1[k], N0[k] + N1[k]) for k in range(M + 1)],
            "forecast_frequency": [div(N0[k] + N1[k], N) for k in range(M + 1)], "pod": pod[:M + 1],
            "pofd": pofd[:M + 1]}


def report(acc, band_w, M, n_thresholds):
    """``acc [S, H, 1 + T 2 (M + 1)]`` and band weights ``[R, H]`` -> ``SCORES`` ``[S, R, T]``, ``CURVES``
    ``[S, R, T, M + 1]`` and ``valid [S, R]`` (the weighted valid cells), float64; the weighted rows are summed one by
    one, in row order; NaN past a source's thresholds"""
    wb = np.asarray(band_w, np.float64)
    R, H = wb.shape
    nV, joint = split(np.asarray(acc), M)
    S, T = joint.shape[0], joint.shape[2]
    out = {k: np.full((S, R, T), np.nan) for k in SCORES}
    out.update({k: np.full((S, R, T, M + 1), np.nan) for k in CURVES})
    out["valid"] = np.zeros((S, R))
    for s in range(S):
        for r in range(R):
            for h in range(H):
                out["valid"][s, r] += wb[r, h] * float(nV[s, h])
            for j in range(n_thresholds[s]):
                N = np.zeros((2, M + 1))
                for h in range(H):
                    N += wb[r, h] * joint[s, h, j].astype(np.float64)
                for k, v in scores_of(N[0], N[1], M).items():
                    out[k][s, r, j] = v
    return out


def mann_whitney(p, o):
    """the probability that a random event cell has a higher forecast probability than a random non-event cell, ties at
    one half: the area under the ROC curve, from raw per-cell probabilities ``p`` and outcomes ``o`` (0 / 1)"""
    p, o = np.asarray(p, np.float64).reshape(-1), np.asarray(o).reshape(-1).astype(bool)
    pos, neg = p[o], p[~o]
    gt = (pos[:, None] > neg[None, :]).sum()
    eq = (pos[:, None] == neg[None, :]).sum()
    return (float(gt) + 0.5 * float(eq)) / (float(pos.size) * float(neg.size))


def quantile_thresholds(x, valid, direction, qs):
    """thresholds at the quantiles ``qs`` of the valid truth values ``x`` of a source: the value at the quantile (the
    lower one of its two neighbours in the sorted values), moved half-way to the next larger distinct value where there
    is one - towards the smaller one for ``"le"`` -, so that a heavily tied (quantised) field keeps events and
    non-events on both sides; rounded to float32"""
    v = np.sort(np.asarray(x, np.float64)[valid])
    u = np.unique(v)
    out = []
    for q in qs:
        at = v[min(max(int(np.floor(q * (v.size - 1))), 0), v.size - 1)]
        i = int(np.searchsorted(u, at))
        if direction == "ge":
            t = 0.5 * (u[i] + u[i + 1]) if i + 1 < u.size else u[i]
        else:
            t = 0.5 * (u[i] + u[i - 1]) if i > 0 else u[i]
        out.append(float(F32(t)))
    return out
