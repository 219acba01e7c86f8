"""Plain numpy restatement of the ensemble verification (paradis_model_amd/ensemble.py, csrc/ensemble.hip); imports
nothing from the package.

``cell_terms(x, y, dtype)`` forms the per-cell terms in ``dtype``: ``np.float32`` is the restatement, operation for
operation in the kernel's order (numpy's float32 arithmetic is IEEE single, one rounding per operation, never
contracted); ``np.float64`` is the mathematics.  The comparisons ``lo`` / ``eq`` and the validity are exact either way.
``hash32`` / ``ranks`` restate the tie-breaking with the running ensemble ordinal, ``row_sums`` the accumulators of one
update (the doubles summed by numpy in double: another order than the kernel's), ``report`` the host arithmetic with
bands and weights."""
import numpy as np

GOLDEN = np.uint32(0x9E3779B9)


def hash32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def cell_terms(x, y, dtype=np.float32):
    """``x`` ``[M, ...]`` members, ``y`` ``[...]`` truth (float32 values) -> dict of ``A, P, E2, V`` (``dtype``),
    ``lo, eq`` (int64) and ``valid`` (bool), each ``[...]``.  Invalid cells hold whatever the arithmetic gives."""
    M = x.shape[0]
    valid = np.isfinite(y) & np.isfinite(x).all(axis=0)
    lo = (x < y[None]).sum(axis=0).astype(np.int64)
    eq = (x == y[None]).sum(axis=0).astype(np.int64)
    x = x.astype(dtype)
    y = y.astype(dtype)
    rM = np.float32(1.0) / np.float32(M) if dtype is np.float32 else np.float64(1.0) / np.float64(M)
    with np.errstate(all="ignore"):
        A = np.zeros(y.shape, dtype)
        S = np.zeros(y.shape, dtype)
        for i in range(M):
            A = A + np.abs(x[i] - y)
            S = S + x[i]
        P = np.zeros(y.shape, dtype)
        for i in range(M):
            for j in range(i + 1, M):
                P = P + np.abs(x[i] - x[j])
        m = S * rM
        d = m - y
        E2 = d * d
        V = np.zeros(y.shape, dtype)
        for i in range(M):
            t = x[i] - m
            V = V + t * t
    for v in (A, P, E2, V):
        assert v.dtype == dtype
    return {"A": A, "P": P, "E2": E2, "V": V, "lo": lo, "eq": eq, "valid": valid}


def ranks(lo, eq, n, c, C, salt):
    """``lo``, ``eq`` ``[H, W]`` of ensemble ordinal ``n`` and state channel ``c`` of ``C`` -> the rank ``[H, W]``"""
    H, W = lo.shape
    h = np.arange(H, dtype=np.uint64)[:, None]
    w = np.arange(W, dtype=np.uint64)[None, :]
    key = ((np.uint64(n % 2 ** 32) * np.uint64(C) + np.uint64(c)) * np.uint64(H) + h) * np.uint64(W) + w
    key = (key + np.uint64(salt % 2 ** 32) * np.uint64(GOLDEN)) % np.uint64(2 ** 32)
    # (uint64 wraps mod 2^64, which 2^32 divides: the residue mod 2^32 is the kernel's uint32 arithmetic)
    hv = hash32(key.astype(np.uint32)).astype(np.int64)
    return lo + hv % (eq + 1)


def row_sums(fc, truth, M, chan, n0=0, salt=0, dtype=np.float32):
    """one update: ``fc`` ``[G * M, C, H, W]`` member-minor, ``truth`` ``[G, C, H, W]``, ``chan`` the state channels
    chosen, ``n0`` the lead's ensemble count before the update -> ``(real [Cs, H, 4] float64, ints [Cs, H, 2 + M]
    int64, detail)``; ``detail``: per (g, cs) the cell arrays, for the tests' conditions"""
    GM, C, H, W = fc.shape
    G = GM // M
    assert G * M == GM and truth.shape == (G, C, H, W)
    real = np.zeros((len(chan), H, 4), np.float64)
    ints = np.zeros((len(chan), H, 2 + M), np.int64)
    detail = {}
    for g in range(G):
        for cs, c in enumerate(chan):
            t = cell_terms(fc[g * M:(g + 1) * M, c], truth[g, c], dtype)
            ok = t["valid"]
            r = ranks(t["lo"], t["eq"], n0 + g, c, C, salt)
            for k, name in enumerate(("A", "P", "E2", "V")):
                real[cs, :, k] += np.where(ok, t[name].astype(np.float64), 0.0).sum(axis=1)
            ints[cs, :, 0] += ok.sum(axis=1)
            for h in range(H):
                ints[cs, h, 1:] += np.bincount(r[h][ok[h]], minlength=M + 1)
            t["rank"] = r
            detail[(g, cs)] = t
    return real, ints, detail


def report(real, ints, band_w, M):
    """``real`` ``[..., Cs, H, 4]``, ``ints`` ``[..., Cs, H, 2 + M]``, ``band_w`` ``[R, H]`` -> the metrics ``[..., Cs,
    R]`` (``rank_hist``: ``[..., Cs, R, M + 1]``), float64, row by row"""
    wb = np.asarray(band_w, np.float64)
    R, H = wb.shape
    lead = real.shape[:-2]
    N = np.zeros(lead + (R,))
    S = np.zeros(lead + (R, 4))
    hist = np.zeros(lead + (R, M + 1))
    for r in range(R):
        for h in range(H):
            N[..., r] += wb[r, h] * ints[..., h, 0]
            S[..., r, :] += wb[r, h] * real[..., h, :]
            hist[..., r, :] += wb[r, h] * ints[..., h, 1:]
    with np.errstate(all="ignore"):
        mae = S[..., 0] / (M * N)
        out = {"mae_members": mae, "crps": mae - S[..., 1] / (M * M * N),
               "crps_fair": mae - S[..., 1] / (M * (M - 1) * N), "rmse_mean": np.sqrt(S[..., 2] / N),
               "spread": np.sqrt(S[..., 3] / ((M - 1) * N))}
        out["spread_skill"] = np.sqrt((M + 1) / M) * out["spread"] / out["rmse_mean"]
        out["rank_hist"] = hist / N[..., None]
        out["outliers"] = out["rank_hist"][..., 0] + out["rank_hist"][..., M]
    return out
