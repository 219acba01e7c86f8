"""CPU-only: the host side of the forecast writer's layout (paradis_model_amd/encode.py) - the spec tables of the default
configuration, ``regions`` and ``template`` against hand-written cases and the restated loops of tests/encode_oracle.py,
the properties of the BitRound oracle, the oracle's initial state against the reference's own functions (golden
e1_encode.pt), and the argument checks of ``paradis_forecast_encode`` that return before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from paradis_model_amd.config import default_config, feature_layout
from tests import encode_oracle as EO
from tests import forecast_oracle as FO
from tests._util import assert_chk, load_golden, max_rel

LEVELS = list(default_config().features.pressure_levels)


def _spec(**kw):
    from paradis_model_amd.encode import EncodeSpec
    cfg = default_config()
    return cfg, EncodeSpec.from_config(cfg, feature_layout(cfg).output_name_order, cfg.features.pressure_levels, **kw)


# ---------------------------------------------------------------------------------- spec tables
def test_default_spec_tables():
    cfg, spec = _spec()
    names = feature_layout(cfg).output_name_order
    assert len(spec.variables) == 12 and spec.n_planes == 96 and spec.keepbits == 16 and spec.keepbits_code == 16
    assert [v.name for v in spec.variables] == [
        "geopotential", "u_component_of_wind", "v_component_of_wind", "vertical_velocity", "specific_humidity",
        "temperature", "10m_u_component_of_wind", "10m_v_component_of_wind", "2m_temperature",
        "mean_sea_level_pressure", "total_precipitation_6hr", "dewpoint_depression"]
    assert [v.levels for v in spec.variables] == [13] * 6 + [1] * 5 + [13]
    assert spec.shadowed == [f"wind_z_h{l}" for l in LEVELS]
    by_name = {v.name: v for v in spec.variables}
    assert [names[c] for c in by_name["vertical_velocity"].sources] == [f"vertical_velocity_h{l}" for l in LEVELS]
    assert [names[c] for c in by_name["u_component_of_wind"].sources] == [f"wind_x_h{l}" for l in LEVELS]
    assert names[by_name["10m_v_component_of_wind"].sources[0]] == "wind_y_10m"
    assert by_name["dewpoint_depression"].sources == tuple(-1 - l for l in range(13))
    written = {names[s] for s in spec.table["src"] if s >= 0}
    assert "wind_z_10m" not in written and not written & set(spec.shadowed)
    assert written | set(spec.shadowed) | {"wind_z_10m"} == set(names)          # every channel is accounted for
    # the same groups as the restated loops of the oracle
    want = EO.variable_indices(cfg, names, LEVELS)
    assert list(want) == [v.name for v in spec.variables[:-1]]
    for v in spec.variables[:-1]:
        kind, ind = want[v.name]
        assert (kind == "sfc") == v.surface and list(v.sources) == (ind if kind == "atm" else [ind])


@pytest.mark.parametrize("shape", [(2, 3, 8, 16), (1, 1, 5, 6)])
def test_block_offsets_are_dense_and_disjoint(shape):
    _, spec = _spec()
    B, n_td, H, W = shape
    P = H * W
    blocks = sorted(spec.block(v, *shape) for v in spec.variables)
    assert blocks[0][0] == 0 and all(a + m == b for (a, m), (b, _) in zip(blocks, blocks[1:]))
    assert blocks[-1][0] + blocks[-1][1] == spec.numel(*shape) == 96 * B * n_td * P
    # every plane of every (sample, slot) lands on its own P elements, by the kernel's address expression
    seen = np.zeros(spec.numel(*shape) // P, np.int32)
    for row in spec.table:
        for b in range(B):
            for t in range(n_td):
                seen[row["first"] * B * n_td + (b * n_td + t) * row["levels"] + row["level"]] += 1
    assert (seen == 1).all()
    # and the views name exactly those blocks
    buf = np.arange(spec.numel(*shape), dtype=np.float32)
    views = spec.views(buf, *shape)
    for v in spec.variables:
        a, m = spec.block(v, *shape)
        assert views[v.name].shape == ((B, n_td, H, W) if v.surface else (B, n_td, v.levels, H, W))
        assert views[v.name].reshape(-1)[0] == a and views[v.name].reshape(-1)[-1] == a + m - 1
        assert np.shares_memory(views[v.name], buf)
    tviews = spec.views(torch.from_numpy(buf), *shape)
    assert all(np.array_equal(tviews[k].numpy(), views[k]) for k in views)
    with pytest.raises(ValueError):
        spec.views(buf[:-1], *shape)


def test_spec_variants_and_refusals():
    from paradis_model_amd.encode import EncodeSpec
    cfg, spec = _spec(dewpoint=False, keepbits="off")
    assert len(spec.variables) == 11 and spec.n_planes == 83 and spec.keepbits is None and spec.keepbits_code == 0
    assert _spec(keepbits=None)[1].keepbits is None and _spec(keepbits=23)[1].keepbits_code == 23
    names = feature_layout(cfg).output_name_order
    for bad in (0, 24, -1, 16.0, True):
        with pytest.raises(ValueError, match="keepbits"):
            EncodeSpec.from_config(cfg, names, LEVELS, keepbits=bad)
    with pytest.raises(ValueError, match="not among"):
        EncodeSpec.from_config(cfg, names[:-1], LEVELS)
    with pytest.raises(ValueError, match="unique"):
        EncodeSpec.from_config(cfg, names + names[:1], LEVELS)
    # float levels name the same channels; no duplicate names: nothing shadowed
    assert EncodeSpec.from_config(cfg, names, [float(l) for l in LEVELS]).table.tobytes() == _spec()[1].table.tobytes()
    cfg.features.output.atmospheric = [v for v in cfg.features.output.atmospheric if v != "vertical_velocity"]
    plain = EncodeSpec.from_config(cfg, names, LEVELS)
    assert plain.shadowed == [] and len(plain.variables) == 12
    by_name = {v.name: v for v in plain.variables}
    assert [names[c] for c in by_name["vertical_velocity"].sources] == [f"wind_z_h{l}" for l in LEVELS]


# ---------------------------------------------------------------------------------- regions and template
def test_regions_hand_written_cases():
    from paradis_model_amd.encode import pred_slice, regions
    pos = np.arange(10)                                       # times already ascending
    # unsorted samples, consecutive after sorting: one run, rows reorder the batch
    (r,) = regions([5, 3, 4], pos, 0, 2)
    assert r.rows.tolist() == [1, 2, 0] and r.time == slice(3, 6) and r.prediction_timedelta == slice(0, 3)
    # a gap in the sorted positions: two runs
    a, b = regions([7, 2, 3, 8], pos, 4, 3)
    assert a.rows.tolist() == [1, 2] and a.time == slice(2, 4) and a.prediction_timedelta == slice(5, 8)
    assert b.rows.tolist() == [0, 3] and b.time == slice(7, 9) and b.prediction_timedelta == slice(5, 8)
    # a dataset whose times are not ascending: positions come from the sort
    times = np.array([30, 10, 20, 0], dtype="datetime64[h]")
    _, pos2 = EO.sorted_time_info(times)
    assert pos2.tolist() == [3, 1, 2, 0]
    got = regions([0, 1, 2, 3], pos2, 0, 1)                   # positions 3, 1, 2, 0: only 1 -> 2 is a step of +1
    assert [(g.rows.tolist(), g.time) for g in got] == [([0], slice(3, 4)), ([1, 2], slice(1, 3)), ([3], slice(0, 1))]
    (one,) = regions([2], pos, 2, 1)
    assert one.rows.tolist() == [0] and one.time == slice(2, 3) and one.prediction_timedelta == slice(3, 4)
    assert pred_slice(0, 2) == slice(0, 3) and pred_slice(0, 2, with_init=False) == slice(1, 3)
    assert pred_slice(2, 1) == slice(3, 4)
    # and the oracle's restatement, over a sweep
    g = np.random.default_rng(5)
    for _ in range(20):
        idx = g.choice(12, size=int(g.integers(1, 7)), replace=False)
        pos3 = g.permutation(12)
        start, n = int(g.integers(0, 4)), int(g.integers(1, 4))
        want = EO.regions(idx, pos3, start, n)
        got = regions(idx, pos3, start, n)
        assert [(r.rows.tolist(), (r.time.start, r.time.stop),
                 (r.prediction_timedelta.start, r.prediction_timedelta.stop)) for r in got] == want


def test_template_hand_written_cases():
    cfg, spec = _spec()
    t = spec.template(n_time=7, forecast_steps=40, output_frequency=2, H=8, W=16)
    assert t["total_pred_steps"] == 21 and t["keepbits"] == 16 and len(t["variables"]) == 12
    assert t["variables"]["temperature"] == {
        "dims": ("time", "prediction_timedelta", "level", "latitude", "longitude"), "shape": (7, 21, 13, 8, 16),
        "chunks": (1, 10, 13, 8, 16)}
    assert t["variables"]["2m_temperature"] == {
        "dims": ("time", "prediction_timedelta", "latitude", "longitude"), "shape": (7, 21, 8, 16),
        "chunks": (1, 10, 8, 16)}
    assert t["variables"]["dewpoint_depression"]["shape"] == (7, 21, 13, 8, 16)
    t = spec.template(n_time=3, forecast_steps=5, output_frequency=2, H=5, W=6)     # min(10, total) = total
    assert t["total_pred_steps"] == 4 and t["variables"]["geopotential"]["chunks"] == (1, 4, 13, 5, 6)
    assert spec.template(1, 1, 1, 4, 4)["total_pred_steps"] == 2
    assert spec.template(1, 9, 1, 4, 4)["variables"]["temperature"]["chunks"][1] == 10      # total = 10
    names = feature_layout(cfg).output_name_order
    for (S, f) in ((40, 2), (5, 2), (1, 1), (12, 3)):
        want, total = EO.template(cfg, names, LEVELS, 7, S, f, 8, 16)
        got = spec.template(7, S, f, 8, 16)
        assert got["total_pred_steps"] == total and list(got["variables"]) == list(want)
        for k, (nd, shape, chunks) in want.items():
            assert (len(got["variables"][k]["dims"]), got["variables"][k]["shape"], got["variables"][k]["chunks"]) == \
                (nd, shape, chunks)


# ---------------------------------------------------------------------------------- BitRound oracle
def _special_bits():
    return np.array([0x7FFFFFFF, 0x7FC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF,
                     0x7F7FFFFF, 0x3F800040, 0x3F800140, 0x3F8000C0, 0x3F80003F, 0x3F800041], dtype=np.uint32)


def test_bitround_oracle_properties():
    g = np.random.default_rng(3)
    x = np.concatenate([g.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** g.integers(-20, 20, 4000),
                        _special_bits().view(np.float32)]).astype(np.float32)
    for keep in (16, 1, 7, 22):
        r = EO.bitround(x, keep)
        assert np.array_equal(EO.bits(EO.bitround(r, keep)), EO.bits(r))                     # idempotent
        assert (EO.bits(r) & ((1 << (23 - keep)) - 1) == 0).all()                             # the dropped bits are zero
    assert np.array_equal(EO.bits(EO.bitround(x, 23)), EO.bits(x)) and np.array_equal(EO.bits(EO.bitround(x, None)), EO.bits(x))
    assert EO.bitround(x, 16) is not x and np.array_equal(EO.bits(x[-14:]), _special_bits().view(np.int32))   # a copy
    # monotone on finite positives
    pos = np.sort(np.abs(x[np.isfinite(x) & (x != 0)]))
    for keep in (16, 1):
        r = EO.bitround(pos, keep)
        assert (np.diff(r[np.isfinite(r)].astype(np.float64)) >= 0).all()
    # relative error <= 2^-17 at keepbits 16 (normal numbers)
    normal = x[np.isfinite(x) & (np.abs(x) >= np.finfo(np.float32).tiny) & (np.abs(x) < 1e38)].astype(np.float64)
    r = EO.bitround(normal.astype(np.float32), 16).astype(np.float64)
    assert np.max(np.abs(r - normal) / np.abs(normal)) <= 2.0 ** -17
    # ties to even at keepbits 16 (maskbits 7: a tail of exactly 0x40 is a tie)
    tie = np.array([0x3F800040, 0x3F8000C0, 0x3F800140, 0x3F800041, 0x3F80003F], np.uint32).view(np.float32)
    assert EO.bits(EO.bitround(tie, 16)).tolist() == [0x3F800000, 0x3F800100, 0x3F800100, 0x3F800080, 0x3F800000]
    # a carry runs into the exponent (and, from the largest patterns, into the sign): still just arithmetic on the bits
    top = np.array([0x7F7FFFFF, 0x7FFFFFFF, 0x7FC00000, 0x7F800000, 0x00000001], np.uint32).view(np.float32)
    assert EO.bits(EO.bitround(top, 16)).view(np.uint32).tolist() == [0x7F800000, 0x80000000, 0x7FC00000, 0x7F800000, 0]


# ---------------------------------------------------------------------------------- the initial state
@pytest.mark.parametrize("grid", ["8x16", "9x16"])
def test_oracle_initial_state_vs_reference_golden(grid):
    g = load_golden("e1_encode.pt")
    rec, names, levels = g["cases"][grid], g["names"], g["levels"]
    cfg = default_config()
    assert names == feature_layout(cfg).output_name_order and levels == LEVELS
    ins, outs = EO.feature_lists(cfg)
    assert ins == g["input_names"] and outs == names
    H, W = rec["H"], rec["W"]
    assert EO.store_features(cfg, rec["seed"]) == rec["features"]
    store = EO.raw_store(rec["seed"] + 10, rec["features"], g["T"], H, W)
    assert_chk([store], rec["chk"])
    rows = EO.init_rows(g["base"], g["n_time_inputs"], g["interval_steps"], g["indices"])
    assert rows == rec["rows"]
    lat, lon = FO.grid_deg(H, W, rec["poles"], np.float64)
    init, dew = EO.initial_state(store.numpy(), rec["features"], rows, ins, outs, levels, lat, lon)
    want, wdew = rec["init"].numpy(), rec["dew"].numpy()
    assert init.shape == want.shape == (2, 1, 97, H, W) and dew.shape == wdew.shape == (2, 1, 13, H, W)
    nan = [names.index(f) for f in rec["nan_channels"]]
    assert rec["nan_channels"] == [f"vertical_velocity_h{l}" for l in levels] + ["total_precipitation_6hr"]
    assert np.isnan(init[:, :, nan]).all() and np.isnan(want[:, :, nan]).all()
    keep = [c for c in range(97) if c not in nan]
    assert np.isfinite(init[:, :, keep]).all()
    for c in keep:
        e = max_rel(torch.from_numpy(init[:, :, c]), torch.from_numpy(want[:, :, c]))
        assert e <= 1e-6, (names[c], e)
    untouched = [c for c in keep if FO.base_name(names[c]) not in ("wind_x", "wind_y", "wind_z", "wind_x_10m", "wind_y_10m")]
    assert np.array_equal(init[:, :, untouched], want[:, :, untouched])            # a gather: the store's bits
    assert max_rel(torch.from_numpy(dew), torch.from_numpy(wdew)) <= 1e-6


# ---------------------------------------------------------------------------------- the C entry point's refusals
def _table():
    _, spec = _spec()
    return spec.table, spec.table.ctypes.data


def _encode(*, chunk_bs=None, chunk_ts=None, dew_bs=None, dew_ts=None, planes=True, out_elems=None, B=2, n=1, C=97,
            L=13, H=8, W=16, n_td=2, td_off=1, keepbits=16, dew=True):
    """paradis_forecast_encode with never-dereferenced data pointers: the checks fire before anything is touched"""
    from paradis_model_amd import _lib
    table, host = _table()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    P = H * W
    cts = C * P if chunk_ts is None else chunk_ts
    dts = L * P if dew_ts is None else dew_ts
    return _lib.lib.paradis_forecast_encode(
        p, n * cts if chunk_bs is None else chunk_bs, cts, p if dew else None, n * dts if dew_bs is None else dew_bs,
        dts, p if planes else None, host if planes else None, len(table), p,
        B * n_td * 96 * P if out_elems is None else out_elems, B, n, C, L, H, W, n_td, td_off, keepbits, None)


def test_forecast_encode_argument_validation_without_gpu():
    from paradis_model_amd import _lib
    for bad in (-1, 24, 99):
        assert _encode(keepbits=bad) == 1
        assert "keepbits" in _lib.last_error()
    assert _encode(n=2, n_td=2, td_off=1) == 1                       # td_off + n > n_td
    assert "slots" in _lib.last_error()
    assert _encode(td_off=-1) == 1
    assert _encode(chunk_ts=97 * 128 - 1) == 1                        # strides shorter than a state
    assert "strides" in _lib.last_error()
    assert _encode(n=2, n_td=3, chunk_bs=97 * 128) == 1               # batch stride shorter than the n states of a sample
    assert _encode(dew_ts=13 * 128 - 4) == 1
    assert "dew" in _lib.last_error()
    assert _encode(planes=False) == 1                                 # a null table
    assert "table" in _lib.last_error()
    assert _encode(C=96) == 1                                         # a row reads channel 96 of a 96-channel chunk
    assert "row" in _lib.last_error()
    assert _encode(dew=False) == 1                                    # a dew row without a dew chunk
    assert _encode(L=12) == 1
    assert _encode(out_elems=2 * 2 * 96 * 128 - 1) == 1               # the buffer is one element short
    assert "buffer" in _lib.last_error()
    assert _encode(H=0) == 1
    # B == 0 does nothing and succeeds, for every keepbits the entry point accepts
    for keep in (0, 1, 16, 23):
        assert _encode(B=0, keepbits=keep) == 0
    assert _lib.lib.paradis_abi_version() == 10                       # additive: the ABI version stays
