"""CPU: the quantile climatology's definition and host side (paradis_model_amd/climatology.py ``build_quantiles``,
``QuantileClimatology``, ``quantile_event``; csrc/quantile.hip's argument checks).

- tests/quantile_oracle.py, the numpy restatement the GPU tests compare against bit for bit, against
  ``np.quantile(float64, method="linear")`` rounded to float32: within 1 float32 ulp (numpy changes its lerp form at
  ``t >= 0.5``, which moves a rare result by one ulp; both are exact to the last rounding otherwise).
- ``build_quantiles``' refusals, each naming the offending thing; the C entry points' checks, which come before any HIP
  call; header, signature table and library agree.
- ``field()`` / ``quantile_event()`` on CPU tensors.
- Through tests/events_oracle.py: an anomaly source at threshold 0 against a per-cell field ``q`` decides exactly
  ``x >= q`` (``x <= q`` for ``"le"``), with ``x == q``, ``x`` one ulp on either side and denormal differences."""
import os
import re

import numpy as np
import pytest
import torch

from tests import events_oracle as EO
from tests import quantile_oracle as QO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("paradis_clim_quantile_max_entries", "paradis_clim_quantile_cells", "paradis_clim_quantile",
               "paradis_clim_quantile_packed")
LEVELS = [0.0, 0.01, 1.0 / 3.0, 0.5, 0.95, 1.0]
NAMES = ["temperature_h500", "temperature_h850", "wind_x_h500", "wind_x_h850", "wind_y_h500", "wind_y_h850",
         "wind_z_h500", "wind_z_h850", "total_precipitation_6hr"]
PLEVELS = [500, 850]


def _C():
    from paradis_model_amd import climatology
    return climatology


def _ordered(a):
    """float32 -> int64 whose order and spacing are the floats' (one ulp == 1)"""
    b = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def _data(kind, n, rng):
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "temperature":
        return (np.float32(250.0) + np.float32(15.0) * x).astype(np.float32)
    if kind == "wind":
        return (np.float32(10.0) * x).astype(np.float32)
    wet = rng.random(n) < 0.35                                          # precipitation: at least 60 % exact zeros
    return np.where(wet, np.abs(x) * np.float32(1e-3), np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("kind", ["temperature", "wind", "precipitation"])
def test_oracle_within_one_ulp_of_numpy_linear(kind):
    rng = np.random.default_rng({"temperature": 11, "wind": 12, "precipitation": 13}[kind])
    worst, zeros, total = 0, 0, 0
    for n in range(1, 301):
        v = _data(kind, n, rng)
        zeros += int((v == 0).sum())
        total += n
        got = np.array(QO.cell_quantiles(v, LEVELS), np.float32)
        want = np.quantile(v.astype(np.float64), LEVELS, method="linear").astype(np.float32)
        assert got.dtype == np.float32 and bool(np.isfinite(got).all())
        assert got[0] == v.min() and got[-1] == v.max()
        worst = max(worst, int(np.abs(_ordered(got) - _ordered(want)).max()))
    print(f"QUANTILE oracle | {kind} | worst distance from np.quantile {worst} ulp | zeros {zeros / total:.2f}")
    if kind == "precipitation":
        assert zeros >= 0.6 * total
    assert worst <= 1


def test_oracle_skips_non_finite_reads_minus_zero_as_zero_and_counts():
    nan, inf = float("nan"), float("inf")
    v = np.array([3.0, nan, 1.0, inf, -inf, 2.0], np.float32)
    assert [float(x) for x in QO.cell_quantiles(v, [0.0, 0.5, 1.0])] == [1.0, 2.0, 3.0]
    assert float(QO.cell_quantiles(v, [0.25])[0]) == 1.5
    assert np.isnan(QO.cell_quantiles(v, [0.5], min_count=4)[0]) and float(QO.cell_quantiles(v, [0.5], 3)[0]) == 2.0
    assert all(np.isnan(x) for x in QO.cell_quantiles(np.array([nan, inf], np.float32), [0.0, 1.0]))
    z = QO.cell_quantiles(np.array([-0.0, -0.0, 0.0], np.float32), [0.0, 0.5, 1.0])
    assert all(x == 0 and not np.signbit(x) for x in z)
    out = QO.slot_quantiles(np.arange(24, dtype=np.float32).reshape(6, 1, 2, 2), [[0, 5, 2], [], [(4, 1.0)]], [0],
                            [0.0, 0.5])
    assert out.shape == (2, 3, 1, 2, 2) and out.dtype == np.float32
    assert np.array_equal(out[:, 0, 0, 0, 0], [0.0, 8.0]) and bool(np.isnan(out[:, 1]).all())
    assert np.array_equal(out[:, 2, 0, 1, 1], [19.0, 19.0])


# ---------------------------------------------------------------------------------- the host side
def _cpu_store(times, feats, grid=(3, 4)):
    from paradis_model_amd.dataset import DeviceStore
    H, W = grid
    F = len(feats)
    st = {k: np.ones(F, np.float32) for k in ("mean", "std", "min", "max")}
    return DeviceStore(np.zeros((len(times), F, H, W), np.float32), times, feats, st, np.linspace(-60, 60, H),
                       np.arange(W) * (360.0 / W), np.zeros((H, W, 1), np.float32), toa_mean=0.0, toa_std=1.0,
                       device="cpu")


def _spec(**kw):
    from paradis_model_amd.forecast import PostSpec
    C = len(NAMES)
    return PostSpec.from_features(NAMES, PLEVELS, zscore_mean=np.zeros(C, np.float32),
                                  zscore_std=np.ones(C, np.float32), custom_normalization=False, dewpoint=False, **kw)


def test_build_quantiles_refuses_on_the_host():
    C = _C()
    times = np.arange(np.datetime64("2020-01-01T00", "h"), np.datetime64("2020-01-03T00", "h"),
                      np.timedelta64(12, "h")).astype("datetime64[us]")
    store = _cpu_store(times, NAMES)
    plan = C.ClimPlan(store.times_us)
    ok = ["temperature_h500", "total_precipitation_6hr"]
    with pytest.raises(ValueError, match="gaussian.*unweighted"):
        C.build_quantiles(store, C.ClimPlan(store.times_us, window_days=5, weights="gaussian", sigma_days=1.5), 0.5,
                          names=ok)
    with pytest.raises(ValueError, match="wind_y_h850.*wind triple"):
        C.build_quantiles(store, plan, 0.5, _spec(), names=["temperature_h500", "wind_y_h850"])
    with pytest.raises(ValueError, match="wind_x_h500"):
        C.build_quantiles(store, plan, 0.5, _spec())                      # the spec's own names hold the winds
    with pytest.raises(ValueError, match="1.5"):
        C.build_quantiles(store, plan, [0.5, 1.5], names=ok)
    with pytest.raises(ValueError, match="-0.1"):
        C.build_quantiles(store, plan, -0.1, names=ok)
    with pytest.raises(ValueError, match="nan"):
        C.build_quantiles(store, plan, [float("nan")], names=ok)
    with pytest.raises(ValueError, match="0.25.*twice"):
        C.build_quantiles(store, plan, [0.25, 0.5, 0.25], names=ok)
    with pytest.raises(ValueError, match="9 levels"):
        C.build_quantiles(store, plan, np.linspace(0, 1, 9), names=ok)
    with pytest.raises(ValueError, match="0 levels"):
        C.build_quantiles(store, plan, [], names=ok)
    with pytest.raises(ValueError, match="geopotential_h500"):
        C.build_quantiles(store, plan, 0.5, names=["temperature_h500", "geopotential_h500"])
    with pytest.raises(ValueError, match="other times"):
        C.build_quantiles(store, C.ClimPlan(store.times_us[:3]), 0.5, names=ok)
    with pytest.raises(ValueError, match="min_count"):
        C.build_quantiles(store, plan, 0.5, names=ok, min_count=0)
    with pytest.raises(ValueError, match="PostSpec or names"):
        C.build_quantiles(store, plan, 0.5)
    with pytest.raises(ValueError, match="no CPU fallback"):              # everything else in order: the device is needed
        C.build_quantiles(store, plan, [0.05, 0.95], names=ok)
    with pytest.raises(ValueError, match="no CPU fallback"):              # a spec without winds keeps every name
        C.build_quantiles(store, plan, [0.05, 0.95], _spec(winds=False))


def test_build_quantiles_refuses_a_list_longer_than_the_maximum():
    C = _C()
    longest = C.max_quantile_entries()
    times = (np.datetime64("2001-01-01T00", "h") + 24 * np.arange(13 * 365).astype("timedelta64[h]")) \
        .astype("datetime64[us]")
    store = _cpu_store(times, ["temperature_h500"], grid=(1, 2))
    plan = C.ClimPlan(store.times_us, days=[40, 100], window_days=365)
    n = int(plan.entries.max())
    assert n > longest
    k = int(np.argmax(plan.entries))
    with pytest.raises(ValueError, match=rf"slot {k} \(day of year {plan.days[k]}, hour 0\) has {n} entries"):
        C.build_quantiles(store, plan, 0.5, names=["temperature_h500"])


def _declared():
    text = open(os.path.join(ROOT, "include", "paradis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(paradis_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_signatures_and_library_agree_for_the_new_symbols():
    from ctypes import c_double, c_float, c_int, c_int64, c_void_p
    from paradis_model_amd import _lib
    declared = _declared()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/paradis_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is declared but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        res, args = _lib.SIGNATURES[name]
        assert res is c_int
        params = [p.strip() for p in declared[name].split(",") if p.strip() != "void"]
        want = []
        for p in params:
            kind = p.rsplit(" ", 1)[0].replace("const ", "").strip()
            want.append(c_void_p if "*" in p else {"int": c_int, "int64_t": c_int64, "float": c_float,
                                                   "double": c_double}[kind])
        assert list(args) == want, f"{name}: signature table {args} against the header's {params}"
    assert _lib.lib.paradis_abi_version() == 10


def test_tile_sizes():
    from paradis_model_amd import _lib
    lib = _lib.lib
    assert lib.paradis_clim_quantile_max_entries() >= 4096
    assert _C().max_quantile_entries() == lib.paradis_clim_quantile_max_entries()
    cells = [lib.paradis_clim_quantile_cells(n) for n in (1, 256, 257, 4096)]
    for c in cells:
        assert c >= 1 and c & (c - 1) == 0, cells                         # a power of two
    assert cells == sorted(cells, reverse=True)                          # longer lists never get more cells
    assert cells[-1] * 4096 * 4 <= 160 * 1024                            # the longest tile fits a CU's LDS


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """rc 1 before any HIP call"""
    from paradis_model_amd import _lib
    lib = _lib.lib
    one = 64      # a non-NULL address that is never dereferenced: every call below is refused or does nothing
    q = np.array([0.0, 0.5, 1.0], np.float64)
    qp = q.ctypes.data

    def call(store=one, T=4, N=0, K=1, max_entries=8, C=1, qptr=qp, Q=3, min_count=1, rows=one, out=one):
        return lib.paradis_clim_quantile(store, T, 1, 2, 2, one, rows, N, K, max_entries, one, C, qptr, Q, min_count,
                                         out, one, None)

    assert call(T=0) == 1
    assert "bad shape" in _lib.last_error()
    assert call(store=None) == 1                                                                  # no store
    assert "pointers required" in _lib.last_error()
    assert call(N=3, rows=None) == 1                                                              # entries, no rows
    assert call(N=-1) == 1
    assert call(Q=9) == 1
    assert "9 levels" in _lib.last_error()
    assert call(Q=-1) == 1
    assert call(qptr=None) == 1
    bad = np.array([0.5, 1.25], np.float64)
    assert call(qptr=bad.ctypes.data, Q=2) == 1
    assert "level 1 is 1.25" in _lib.last_error()
    nan = np.array([float("nan")], np.float64)
    assert call(qptr=nan.ctypes.data, Q=1) == 1
    assert call(max_entries=lib.paradis_clim_quantile_max_entries() + 1) == 1
    assert "max_entries" in _lib.last_error()
    assert call(max_entries=-1) == 1
    assert call(min_count=0) == 1
    assert "min_count" in _lib.last_error()
    assert call(out=None) == 1
    assert call(K=0) == 0 and call(C=0) == 0 and call(Q=0) == 0                                   # nothing to do
    assert lib.paradis_clim_quantile_packed(one, None, one, 4, 1, 2, 2, one, one, 0, 1, 8, one, 1, qp, 3, 1, one, one,
                                            None) == 1
    assert lib.paradis_clim_quantile_packed(one, one, one, 4, 1, 2, 2, one, one, 0, 0, 8, one, 1, qp, 3, 1, one, one,
                                            None) == 0


def test_field_level_and_quantile_event_on_cpu_tensors():
    C = _C()
    Q, K, H, W = 2, 3, 2, 5
    names = ["total_precipitation_6hr", "temperature_h850"]
    data = torch.arange(Q * K * len(names) * H * W, dtype=torch.float32).reshape(Q, K, len(names), H, W)
    times = np.arange(np.datetime64("2020-01-01T00", "h"), np.datetime64("2020-01-04T00", "h"),
                      np.timedelta64(24, "h")).astype("datetime64[us]")
    plan = C.ClimPlan(times.astype(np.int64), days=[1, 2, 3])
    qc = C.QuantileClimatology(data, plan, names, [0.1, 0.9])
    assert qc.levels == [0.1, 0.9] and qc.names == names and qc.plan is plan
    assert qc.level(0.9).data_ptr() == data[1].data_ptr() and tuple(qc.level(0.1).shape) == (K, 2, H, W)
    with pytest.raises(ValueError, match="0.5"):
        qc.level(0.5)
    idx = qc.index(times[[2, 0]])
    assert idx.dtype == torch.int32 and idx.tolist() == [2, 0]
    f = qc.field(NAMES, {"temperature_h850": 0.1, "total_precipitation_6hr": 0.9})
    assert tuple(f.shape) == (K, len(NAMES), H, W) and f.dtype == torch.float32 and f.is_contiguous()
    assert torch.equal(f[:, NAMES.index("temperature_h850")], data[0, :, 1])
    assert torch.equal(f[:, NAMES.index("total_precipitation_6hr")], data[1, :, 0])
    rest = [c for c, n in enumerate(NAMES) if n not in names]
    assert bool(torch.isnan(f[:, rest]).all()) and int(torch.isnan(f).sum()) == K * len(rest) * H * W
    assert bool(torch.isnan(qc.field(NAMES, {"temperature_h850": 0.9})[:, NAMES.index("total_precipitation_6hr")]).all())
    with pytest.raises(ValueError, match="wind_x_h500"):
        qc.field(NAMES, {"wind_x_h500": 0.1})                             # a state name without quantiles
    with pytest.raises(ValueError, match="geopotential"):
        qc.field(NAMES, {"geopotential": 0.1})
    with pytest.raises(ValueError, match="0.5"):
        qc.field(NAMES, {"temperature_h850": 0.5})
    assert C.quantile_event("temperature_h850") == {"source": ("anomaly", "temperature_h850"), "thresholds": [0.0],
                                                    "direction": "ge"}
    assert C.quantile_event("total_precipitation_6hr", "le")["direction"] == "le"
    with pytest.raises(ValueError, match="direction"):
        C.quantile_event("temperature_h850", "gt")
    # the entry is what the tables' parser takes
    from paradis_model_amd.events import parse_events
    got = parse_events("test", {"cold": C.quantile_event("temperature_h850", "le")}, NAMES, True)
    assert got["n_thresholds"] == [1] and got["directions"] == ["le"] and got["thresholds"] == [[0.0]]


def test_anomaly_at_zero_decides_x_ge_q_exactly():
    """x - q >= 0 <=> x >= q in fp32 without flush to zero: ties, neighbours one ulp away, denormal differences"""
    rng = np.random.default_rng(5)
    B, H, W = 4, 8, 64
    q = np.empty((H, W), np.float32)
    q[0:2] = (250.0 + 15.0 * rng.standard_normal((2, W))).astype(np.float32)         # temperature
    q[2:4] = np.where(rng.random((2, W)) < 0.6, 0.0, np.abs(rng.standard_normal((2, W))) * 1e-3)   # precipitation
    q[4:6] = (rng.standard_normal((2, W)) * 3e-38).astype(np.float32)                 # around the smallest normals
    q[6] = (10.0 * rng.standard_normal(W)).astype(np.float32)
    q[7] = np.nan                                                                   # no quantile: no valid cell
    x = np.empty((2, B, H, W), np.float32)                                          # forecast, truth
    for a in range(2):
        x[a, 0] = q                                                                 # x == q
        x[a, 1] = np.nextafter(q, np.float32(np.inf))                               # one ulp above
        x[a, 2] = np.nextafter(q, np.float32(-np.inf))                              # one ulp below
        x[a, 3] = q + (rng.standard_normal((H, W)) * np.abs(q) * 1e-6).astype(np.float32)
    x[1] = x[1][[1, 2, 3, 0]]                                                       # truth: another order
    x[0, 3, 4:6] = (q[4:6].astype(np.float64) + rng.integers(-40, 41, (2, W)) * 1.4e-45).astype(np.float32)
    diff = x[0].astype(np.float64) - q.astype(np.float64)
    tiny = np.isfinite(diff) & (diff != 0) & (np.abs(diff) < np.finfo(np.float32).tiny)
    assert int(tiny.sum()) >= 200                                                   # denormal differences are there
    assert int((x[0, 0] == q).sum()) == 7 * W
    C, c = 3, 1
    f = np.zeros((B, C, H, W), np.float32)
    t = np.zeros((B, C, H, W), np.float32)
    f[:, c], t[:, c] = x[0], x[1]
    clim = np.full((2, C, H, W), np.nan, np.float32)
    clim[1, c] = q
    index = np.ones(B, np.int64)
    for direction, op in (("ge", np.greater_equal), ("le", np.less_equal)):
        src = [{"kind": "anomaly", "c0": c, "thresholds": [0.0], "direction": direction}]
        got = EO.counts(f, t, src, clim, index)
        valid = np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(q)
        with np.errstate(invalid="ignore"):
            F, O = valid & op(x[0], q), valid & op(x[1], q)                        # no subtraction
        assert np.array_equal(got["valid"][0], valid.sum(axis=(0, 2)))
        assert np.array_equal(got["forecast_yes"][0, :, 0], F.sum(axis=(0, 2)))
        assert np.array_equal(got["observed_yes"][0, :, 0], O.sum(axis=(0, 2)))
        assert np.array_equal(got["both"][0, :, 0], (F & O).sum(axis=(0, 2)))
        assert 0 < int(F.sum()) < int(valid.sum()) and int(got["valid"][0, 7]) == 0
