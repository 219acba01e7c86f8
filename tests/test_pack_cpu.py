"""CPU: the 16-bit plane packing as tests/pack_oracle.py restates it - its error bounds on random planes of every
normalisation kind, the special planes - and what the packed store shows without a device: the symbols, the ABI, the
argument checks of the three entry points and of ``DeviceStore``.

The bounds.  A linear plane decodes within ``0.5 s (1 + 2^-6) + 2^-22 max(|lo|, |hi|)``, s = (hi - lo) / 65534: half a
step, 2^-6 of it for the float32 roundings of the quotient and of s, and the two float32 roundings of the decode.
Precipitation is packed as log(x + 1e-6) and held to ``0.5 s_y (1 + 2^-6) + 2e-5`` in normalised units
(log(x + 1e-6) + 10, where one float32 ulp is 9.5e-7 and the way back and forth rounds a handful of times).
"""
import os

import numpy as np
import pytest

from tests import batch_oracle as BO
from tests import pack_oracle as PK

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("paradis_pack_planes", "paradis_pack_planes_ws_bytes", "paradis_pack_planes_piece",
               "paradis_unpack_planes", "paradis_assemble_batch_packed")

# name -> generator of one plane (rng -> float array); the kinds of the feed's normalisations and the edge ranges
LINEAR_PLANES = {
    "temperature (z-score)": lambda r: 250 + 30 * r.standard_normal(4096),
    "geopotential (z-score)": lambda r: 5e5 + 3e3 * r.standard_normal(4096),
    "humidity": lambda r: np.exp(r.uniform(np.log(1e-6), np.log(3e-2), 4096)),
    "1e-3 wide at 1e5": lambda r: 1e5 + 1e-3 * r.random(4096),
    "15 values": lambda r: -40 + 80 * r.random(15),
    "wide": lambda r: r.standard_normal(4096) * 1e6,
}


@pytest.mark.parametrize("name", list(LINEAR_PLANES))
def test_linear_planes_decode_within_the_bound(name):
    rng = np.random.default_rng(list(LINEAR_PLANES).index(name))
    worst = 0.0
    for _ in range(200):
        x = LINEAR_PLANES[name](rng).astype(f32)
        codes, lo, s = PK.pack_plane(x)
        assert codes.dtype == np.uint16 and codes.max() <= 65534 and codes.min() == 0
        assert lo == x.min() and s == f32(f32(x.max() - x.min()) / f32(65534))
        y = PK.unpack_plane(codes, lo, s)
        err = np.abs(y.astype(np.float64) - x.astype(np.float64)).max()
        bound = PK.linear_bound(x.min(), x.max())
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
    print(f"{name}: worst error / bound {worst:.3f}")


def _precip_plane(rng, n=4096):
    return np.where(rng.random(n) < 0.6, 0.0, np.exp(rng.uniform(np.log(1e-7), np.log(0.2), n))).astype(f32)


def test_precipitation_in_the_log_domain_within_the_bound():
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(200):
        x = _precip_plane(rng)
        codes, lo, s = PK.pack_plane(x, PK.LOG)
        back = PK.unpack_plane(codes, lo, s, PK.LOG)
        assert (back >= 0).all()
        err = np.abs(PK.normalise_precip(back).astype(np.float64) - PK.normalise_precip(x)).max()
        worst = max(worst, err / PK.precip_bound(s))
        assert err <= PK.precip_bound(s), (err, PK.precip_bound(s), float(s))
    print(f"precipitation, log domain: worst error / bound {worst:.3f}")


def test_precipitation_must_not_be_packed_linearly():
    """the reason for the per-feature domain: a linear step of max / 65534 wipes out drizzle"""
    rng = np.random.default_rng(12)
    x = _precip_plane(rng)
    x[0], x[1] = 0.2, 0.0
    lin = PK.unpack_plane(*PK.pack_plane(x))
    log = PK.unpack_plane(*PK.pack_plane(x, PK.LOG), PK.LOG)
    n0 = PK.normalise_precip(x).astype(np.float64)
    err_lin = np.abs(PK.normalise_precip(lin) - n0).max()
    err_log = np.abs(PK.normalise_precip(log) - n0).max()
    assert err_lin > 0.5 and err_log < 2e-4, (err_lin, err_log)


def test_special_planes():
    nan, inf = f32(np.nan), f32(np.inf)
    # constant: s == 0, every code 0, decodes to the constant exactly
    x = np.full(24, 273.15, f32)
    codes, lo, s = PK.pack_plane(x)
    assert s == 0 and lo == f32(273.15) and not codes.any()
    assert np.array_equal(PK.unpack_plane(codes, lo, s), x)
    # all missing: lo = s = 0, every code 65535, decodes to NaN
    codes, lo, s = PK.pack_plane(np.array([nan, inf, -inf, nan], f32))
    assert lo == 0 and s == 0 and (codes == PK.MISSING).all()
    assert np.isnan(PK.unpack_plane(codes, lo, s)).all()
    # one finite value among missing ones: a constant plane of that value
    x = np.array([nan, 7.5, inf], f32)
    codes, lo, s = PK.pack_plane(x)
    assert lo == f32(7.5) and s == 0 and codes.tolist() == [PK.MISSING, 0, PK.MISSING]
    back = PK.unpack_plane(codes, lo, s)
    assert back[1] == f32(7.5) and np.isnan(back[[0, 2]]).all()
    # NaN and both infinities are missing and decode to NaN; the range comes from the finite values alone
    x = np.array([1.0, nan, 3.0, inf, -inf, 2.0], f32)
    codes, lo, s = PK.pack_plane(x)
    assert lo == 1 and s == f32(f32(2.0) / f32(65534))
    assert codes.tolist() == [0, PK.MISSING, 65534, PK.MISSING, PK.MISSING, 32767]
    back = PK.unpack_plane(codes, lo, s)
    assert np.isnan(back[[1, 3, 4]]).all() and np.abs(back[[0, 2, 5]] - x[[0, 2, 5]]).max() <= PK.linear_bound(1, 3)
    # a minimum of 0: zeros come back as zeros, in both domains; -0 is stored as +0
    x = np.array([0.0, 0.05, 0.0, 0.01], f32)
    codes, lo, s = PK.pack_plane(x)
    assert lo == 0 and codes[0] == 0 and PK.unpack_plane(codes, lo, s)[[0, 2]].tolist() == [0.0, 0.0]
    back = PK.unpack_plane(*PK.pack_plane(x, PK.LOG), PK.LOG)
    assert (back >= 0).all() and back[0] <= 1e-12 and back[0] == back[2]
    _, lo, _ = PK.pack_plane(np.array([-0.0, 1.0], f32))
    assert lo == 0 and not np.signbit(lo)
    # the log domain: values at or below -1e-6 have no logarithm and are missing
    codes, _, _ = PK.pack_plane(np.array([-1.0, 0.0, 1.0, -1e-6], f32), PK.LOG)
    assert codes[0] == PK.MISSING and codes[3] == PK.MISSING and codes[1] == 0 and codes[2] == 65534


def test_store_round_trip_matches_the_plane_functions():
    case = BO.build_case(3, 5, n_time_inputs=2, steps=1, n_samples=2, seed=3)
    x = case.store.numpy()
    domains = [PK.LOG if n.startswith("total_precipitation_6hr") else PK.LINEAR for n in case.features]
    assert PK.LOG in domains
    codes, params = PK.pack_store(x, domains)
    assert codes.shape == x.shape and params.shape == x.shape[:2] + (2,)
    back = PK.unpack_store(codes, params, domains)
    for f, d in enumerate(domains):
        for t in range(x.shape[0]):
            if d == PK.LINEAR:
                assert np.abs(back[t, f].astype(np.float64) - x[t, f]).max() <= PK.linear_bound(x[t, f].min(), x[t, f].max())
            else:
                err = np.abs(PK.normalise_precip(back[t, f]).astype(np.float64) - PK.normalise_precip(x[t, f])).max()
                assert err <= PK.precip_bound(params[t, f, 1])


def test_new_symbols_header_and_abi():
    from paradis_model_amd import _lib
    header = open(os.path.join(ROOT, "include", "paradis_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert f"{name}(" in header, name
    assert _lib.lib.paradis_abi_version() == 10
    assert "The 16-bit packed store (ABI 10, additive)" in header
    piece = _lib.lib.paradis_pack_planes_piece()
    assert piece == 8192
    ws = _lib.lib.paradis_pack_planes_ws_bytes
    assert ws(0, 6, 9, 16) == 0 and ws(7, 6, 9, 16) == 7 * 6 * 8
    assert ws(2, 97, 721, 1440) == 2 * 97 * 127 * 8                        # 1 M values: 127 pieces per plane


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from paradis_model_amd import _lib
    lib = _lib.lib
    # pack: shape, rows outside the store, missing pointers
    assert lib.paradis_pack_planes(None, 2, 0, 4, 8, None, 0, 6, None, None, None, None) == 1
    assert "bad shape" in _lib.last_error()
    assert lib.paradis_pack_planes(None, 2, 3, 4, 8, None, 5, 6, None, None, None, None) == 1
    assert "outside a store" in _lib.last_error()
    assert lib.paradis_pack_planes(None, 2, 3, 4, 8, None, -1, 6, None, None, None, None) == 1
    assert lib.paradis_pack_planes(None, 2, 3, 4, 8, None, 0, 6, None, None, None, None) == 1
    assert "pointers required" in _lib.last_error()
    assert lib.paradis_pack_planes(None, 0, 3, 4, 8, None, 0, 6, None, None, None, None) == 0      # n == 0: nothing
    # unpack
    assert lib.paradis_unpack_planes(None, None, None, 6, 3, 0, 8, 0, 2, None, None) == 1
    assert "bad shape" in _lib.last_error()
    for a, b in ((-1, 2), (3, 2), (0, 7)):
        assert lib.paradis_unpack_planes(None, None, None, 6, 3, 4, 8, a, b, None, None) == 1
        assert "outside a store" in _lib.last_error()
    assert lib.paradis_unpack_planes(None, None, None, 6, 3, 4, 8, 0, 2, None, None) == 1
    assert "pointers required" in _lib.last_error()
    assert lib.paradis_unpack_planes(None, None, None, 6, 3, 4, 8, 2, 2, None, None) == 0          # a == b: nothing
    # packed assembly: the checks of paradis_assemble_batch
    def assemble(T=6, F=3, H=4, W=8, B=1, interval=1, n_t=1, Fin=1, S=1, Fout=1, planes=1):
        return lib.paradis_assemble_batch_packed(None, None, None, T, F, H, W, None, B, 0, interval, planes or None,
                                                 n_t, Fin, S, Fout, None, None, 1e-12, None, None)
    for bad in (dict(T=0), dict(F=0), dict(B=-1), dict(n_t=0), dict(S=-1), dict(Fin=0), dict(interval=0),
                dict(planes=0)):
        assert assemble(**bad) == 1, bad
        assert "assemble_batch_packed" in _lib.last_error()
    assert assemble() == 1 and "pointers required" in _lib.last_error()
    assert assemble(B=0) == 0                                                                      # B == 0: nothing


def test_device_store_packing_arguments():
    from paradis_model_amd.dataset import DeviceStore
    case = BO.build_case(4, 6, n_time_inputs=2, steps=1, n_samples=3, seed=5)
    args = (case.store.numpy(), case.times, case.features, case.stats, case.lat, case.lon, case.constants,
            case.toa_mean, case.toa_std)
    with pytest.raises(ValueError, match="HIP device"):
        DeviceStore(*args, device="cpu", packing="u16")
    with pytest.raises(ValueError, match="packing must be"):
        DeviceStore(*args, device="cpu", packing="fp16")
    store = DeviceStore(*args, device="cpu")                               # unchanged: a float32 store
    assert store.packing is None and store.data is not None and store.codes is None
    assert store.nbytes == case.store.numel() * 4 and not store.domain.any()
    assert store.rows(1, 3).data_ptr() == store.data[1:3].data_ptr()       # a view
