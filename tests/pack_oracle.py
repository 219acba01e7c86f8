"""CPU restatement of the 16-bit plane packing (include/paradis_hip.h "The 16-bit packed store", csrc/feed.hip:
``pack_domain_value``, ``pack_code``, ``unpack_value``) in numpy float32, operation by operation.

TEST INFRASTRUCTURE ONLY.  Every intermediate is a float32 array, so each numpy operation is one IEEE float32
operation: the subtraction, the division and ``np.rint`` are exactly the kernel's (it is built with -ffp-contract=off).
The two transcendental steps of the log domain are the correctly rounded float32 ``log`` / ``exp``: evaluated in float64
and rounded once, here as in the kernel.
"""
import numpy as np

f32 = np.float32
MISSING = 65535
TOP = f32(65534.0)
SHIFT = f32(1e-6)
LINEAR, LOG = 0, 1


def domain_value(x, domain):
    """the packed quantity y of a float32 array"""
    x = np.asarray(x, dtype=f32)
    if domain == LOG:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.log((x + SHIFT).astype(f32).astype(np.float64)).astype(f32)
    return x


def pack_plane(x, domain=LINEAR):
    """(codes uint16 like x, lo float32, s float32) of one plane"""
    y = domain_value(x, domain)
    fin = np.isfinite(y)
    if not fin.any():
        return np.full(y.shape, MISSING, np.uint16), f32(0), f32(0)
    lo, hi = f32(y[fin].min()), f32(y[fin].max())
    if lo == 0:
        lo = f32(0.0)                                                   # -0 is stored as +0
    s = f32(f32(hi - lo) / TOP)
    safe = np.where(fin, y, lo).astype(f32)
    if s == 0:
        c = np.zeros(y.shape, f32)
    else:
        c = np.rint(((safe - lo).astype(f32) / s).astype(f32)).astype(f32)
    c = np.minimum(np.maximum(c, f32(0)), TOP)
    codes = c.astype(np.uint16)
    codes[~fin] = MISSING
    return codes, lo, s


def unpack_plane(codes, lo, s, domain=LINEAR):
    """float32 values of one plane: ``lo + s * code`` in two float32 roundings, NaN where missing"""
    c = codes.astype(f32)
    y = (f32(lo) + (f32(s) * c).astype(f32)).astype(f32)
    if domain == LOG:
        with np.errstate(over="ignore"):
            e = np.exp(y.astype(np.float64)).astype(f32)
        y = np.maximum((e - SHIFT).astype(f32), f32(0))
    return np.where(codes == MISSING, f32(np.nan), y).astype(f32)


def pack_store(x, domains):
    """x [T, F, H, W] float32, domains [F] -> (codes uint16 [T, F, H, W], params float32 [T, F, 2])"""
    x = np.asarray(x, dtype=f32)
    T, F = x.shape[:2]
    codes = np.empty(x.shape, np.uint16)
    params = np.empty((T, F, 2), f32)
    for t in range(T):
        for f in range(F):
            codes[t, f], params[t, f, 0], params[t, f, 1] = pack_plane(x[t, f], int(domains[f]))
    return codes, params


def unpack_store(codes, params, domains):
    out = np.empty(codes.shape, f32)
    for t in range(codes.shape[0]):
        for f in range(codes.shape[1]):
            out[t, f] = unpack_plane(codes[t, f], params[t, f, 0], params[t, f, 1], int(domains[f]))
    return out


def linear_bound(lo, hi):
    """decode error bound of a linear plane with finite range [lo, hi]: half a step (with 2^-6 for the rounding of the
    quotient and of s) plus the two float32 roundings of the decode"""
    lo, hi = float(lo), float(hi)
    s = float(f32(f32(f32(hi) - f32(lo)) / TOP))
    return 0.5 * s * (1 + 2.0 ** -6) + 2.0 ** -22 * max(abs(lo), abs(hi))


def precip_bound(s_y):
    """error bound of a log-domain precipitation plane in NORMALISED units (log(x + 1e-6) + 10)"""
    return 0.5 * float(s_y) * (1 + 2.0 ** -6) + 2e-5


def normalise_precip(x):
    """the precipitation normalisation log(x + 1e-6) + 10 in float32, as the feed applies it: the quantity the
    precipitation bound is stated in"""
    return (np.log((np.asarray(x, f32) + SHIFT).astype(f32)).astype(f32) + f32(10)).astype(f32)
