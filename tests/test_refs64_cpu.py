"""The fp64 references of tests/_refs64.py are themselves checked here, without a GPU: against the reference-project
goldens (fp32 results, so 1e-6 max-rel - the level tests/test_oracle_golden.py uses for oracle-versus-golden), against
the fp32 oracle function of the same name at a few shapes, and (AdamW) against torch.optim.AdamW on fp64 parameters."""
import pytest
import torch

from oracle import paradis_oracle as O
from paradis_model_amd.config import default_config
from tests import _refs64 as R
from tests._util import load_golden, max_rel, seeded

GOLD = 1e-6      # fp64 reference vs an fp32 golden
ORACLE = 2e-6    # fp64 reference vs the fp32 oracle at small shapes (both sides' fp32 rounding of short sums)


def _d(t):
    return t.detach().double().clone().requires_grad_(True)


def _check(y, leaves, rec, names=()):
    y.backward(rec["cot"].double())
    assert max_rel(y, rec["y"]) <= GOLD
    assert max_rel(leaves[0].grad, rec["gx"]) <= GOLD
    for n, t in zip(names, leaves[1:]):
        assert max_rel(t.grad, rec["grads"][n]) <= GOLD, n


# ---------------------------------------------------------------------------------------------- goldens
def test_resampling_references_match_the_goldens():
    g = load_golden("g3_blocks.pt")
    seen = 0
    for key, rec in g.items():
        if key.startswith("downsample"):
            x = _d(rec["x"])
            _check(R.avgpool_geo(x, int(key.split("_s")[1])), [x], rec)
        elif key.startswith("upsample"):
            nlat, nlon = map(int, key.split("_")[1].split("x"))
            x = _d(rec["x"])
            _check(R.upsample_lonp(x, nlat, nlon), [x], rec)
        else:
            continue
        seen += 1
    assert seen == 10


def test_channel_norm_reference_matches_the_golden():
    rec = load_golden("g3_blocks.pt")["channelnorm"]
    x, w, b = _d(rec["x"]), _d(rec["params"]["weight"]), _d(rec["params"]["bias"])
    _check(R.channel_norm(x, w, b), [x, w, b], rec, ("weight", "bias"))


@pytest.mark.parametrize("tag", ["noproj", "proj"])
def test_global_bias_reference_matches_the_golden(tag):
    rec = load_golden("g3_blocks.pt")[f"globalbias_{tag}"]
    names = list(rec["params"])
    x = _d(rec["x"])
    P = [_d(rec["params"][n]) for n in names]
    _check(x + R.global_bias_map(*P).unsqueeze(0), [x] + P, rec, names)


def test_loss_reference_matches_the_golden():
    g = load_golden("g6_loss.pt")
    seen = 0
    for key, rec in g.items():
        if "loss" not in rec:
            continue
        nlat, nlon = int(key.split("x")[0]), int(key.split("x")[1].split("_")[0])
        kind = {"mse": 0, "reversed_huber": 1}[key.split("_", 1)[1]]
        p = _d(seeded(rec["pred_seed"], 2, 97, nlat, nlon, scale=1.5))
        t = seeded(rec["target_seed"], 2, 97, nlat, nlon).double()
        l = R.loss(p, t, rec["feature_weights"].double(), rec["lat_weights"].double(), kind, 1.0)
        l.backward()
        assert abs(float(l.detach()) - float(rec["loss"])) <= GOLD * abs(float(rec["loss"])), key
        assert max_rel(p.grad[:, ::8, ::2, ::4], rec["gpred_sub"]) <= GOLD, key
        seen += 1
    assert seen == 4


# ---------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("H,W,s", [(12, 16, 3), (9, 4, 2), (33, 64, 5), (32, 64, 7)])
def test_avgpool_reference_vs_oracle(H, W, s):
    x, ct = seeded(1, 2, 3, H, W), seeded(2, 2, 3, (H - 1) // s + 1, (W - 1) // s + 1)
    xo = x.clone().requires_grad_(True)
    yo = O.avgpool_geo(xo, s)
    yo.backward(ct)
    xr = _d(x)
    yr = R.avgpool_geo(xr, s)
    yr.backward(ct.double())
    assert yr.shape == yo.shape
    assert max_rel(yo, yr) <= ORACLE and max_rel(xo.grad, xr.grad) <= ORACLE


def test_geocyclic_index_reference_is_the_oracle_map():
    for H, W, p in ((12, 16, 2), (9, 4, 2), (33, 64, 2), (4, 4, 2)):
        row, col = O.geocyclic_source_index(H, W, p)
        assert torch.equal(R.geocyclic_index(H, W, p), torch.from_numpy(row * W + col).reshape(-1))


@pytest.mark.parametrize("Hc,Wc,H,W", [(16, 32, 32, 64), (9, 16, 33, 64), (11, 22, 32, 66), (5, 7, 5, 28)])
def test_upsample_reference_vs_oracle(Hc, Wc, H, W):
    x, ct = seeded(1, 2, 3, Hc, Wc), seeded(2, 2, 3, H, W)
    xr = _d(x)
    yr = R.upsample_lonp(xr, H, W)
    yr.backward(ct.double())
    # the same definition through ATen's interpolate, in fp64 (tight) and in fp32 (the oracle as shipped)
    xo = _d(x)
    yo = O.upsample_lon_periodic(xo, H, W)
    yo.backward(ct.double())
    assert max_rel(yr, yo) <= 1e-12 and max_rel(xr.grad, xo.grad) <= 1e-12
    assert max_rel(O.upsample_lon_periodic(x, H, W), yr) <= ORACLE


@pytest.mark.parametrize("B,C,H,W", [(2, 20, 12, 16), (1, 1152, 3, 8), (2, 3, 5, 7)])
def test_channel_norm_reference_vs_oracle(B, C, H, W):
    x, w, b, ct = seeded(1, B, C, H, W, scale=3.0) + 1.0, 1.0 + seeded(2, C, scale=0.2), seeded(3, C), seeded(4, B, C, H, W)
    to = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yo = O.channel_norm(*to)
    yo.backward(ct)
    tr = [_d(t) for t in (x, w, b)]
    yr = R.channel_norm(*tr)
    yr.backward(ct.double())
    assert max_rel(yo, yr) <= ORACLE
    for a, r in zip(to, tr):
        assert max_rel(a.grad, r.grad) <= 5 * ORACLE   # fp32 sums over C (gx) and B*H*W (gw, gb) on the oracle side


@pytest.mark.parametrize("Cin,Co,Rk,H,W", [(8, None, 16, 12, 16), (3, 7, 5, 9, 4), (17, 24, 30, 33, 64)])
def test_global_bias_reference_vs_oracle(Cin, Co, Rk, H, W):
    A, U, V = seeded(1, Cin, Rk, scale=0.5), seeded(2, Rk, H), seeded(3, Rk, W)
    Pw = seeded(4, Co, Cin, scale=0.5) if Co else None
    ct = seeded(5, Co or Cin, H, W)
    ts = [t for t in (A, U, V, Pw) if t is not None]
    to = [t.clone().requires_grad_(True) for t in ts]
    yo = O.global_bias_map(*to, *(() if Co else (None,)))
    yo.backward(ct)
    tr = [_d(t) for t in ts]
    yr = R.global_bias_map(*tr)
    yr.backward(ct.double())
    assert max_rel(yo, yr) <= ORACLE
    for a, r in zip(to, tr):
        assert max_rel(a.grad, r.grad) <= 5 * ORACLE
    assert torch.equal(R.global_bias_m8(*tr[:3]).detach(), R.global_bias_map(*tr[:3]).detach())


@pytest.mark.parametrize("name,code", [("SiLU", 1), ("GELU", 2)])
def test_activation_reference_vs_oracle(name, code):
    x = torch.cat([seeded(1, 700, scale=3.0), torch.linspace(-90, 90, 361), torch.tensor([0.0, -0.0, 1e-30, -1e-30])])
    xo = x.clone().requires_grad_(True)
    yo = O.activation(xo, name)
    yo.backward(torch.ones_like(x))
    xr = _d(x)
    yr = R.act(xr, code)
    yr.backward(torch.ones_like(xr))
    assert max_rel(yo, yr) <= ORACLE and max_rel(xo.grad, xr.grad) <= ORACLE
    assert torch.isfinite(yr).all() and torch.isfinite(xr.grad).all()


def test_gated_blend_and_bias_sum_references_vs_aten():
    h, adv, al, ct = seeded(1, 3, 5, 8, 16), seeded(2, 3, 5, 8, 16), seeded(3, 5), seeded(4, 3, 5, 8, 16)
    to = [t.clone().requires_grad_(True) for t in (h, adv, al)]
    yo = to[0] + torch.sigmoid(to[2]).view(1, -1, 1, 1) * (to[1] - to[0])
    yo.backward(ct)
    tr = [_d(t) for t in (h, adv, al)]
    yr = R.gated_blend(*tr)
    yr.backward(ct.double())
    assert max_rel(yo, yr) <= ORACLE
    for a, r in zip(to, tr):
        assert max_rel(a.grad, r.grad) <= ORACLE
    dz = seeded(5, 3, 5, 128)
    gmap, gb = R.bias_grads(dz.double())
    assert max_rel(dz.sum(0), gmap) <= ORACLE and max_rel(dz.sum((0, 2)), gb) <= ORACLE
    # the definition, element by element
    assert float(gmap[2, 7]) == float(dz[:, 2, 7].double().sum()) and abs(float(gb[4]) - float(dz[:, 4].double().sum())) < 1e-12


@pytest.mark.parametrize("kind", ["mse", "reversed_huber"])
@pytest.mark.parametrize("delta", [0.25, 1.0, 3.0])
@pytest.mark.parametrize("shape,with_wl", [((2, 97, 32, 64), True), ((1, 3, 5, 7), False), ((2, 4, 9, 16), True)])
def test_loss_reference_vs_oracle(kind, delta, shape, with_wl):
    B, C, H, W = shape
    p, t = seeded(1, *shape, scale=1.5), seeded(2, *shape)
    wf = seeded(3, C).abs() + 0.1
    wl = (seeded(4, H).abs() + 0.5) if with_wl else None
    po = p.clone().requires_grad_(True)
    lo = O.paradis_loss(po, t, wf, wl, kind, delta)
    lo.backward()
    pr = _d(p)
    lr = R.loss(pr, t.double(), wf.double(), wl.double() if with_wl else None, {"mse": 0, "reversed_huber": 1}[kind], delta)
    lr.backward()
    assert abs(float(lo) - float(lr)) <= ORACLE * abs(float(lr))
    assert max_rel(po.grad, pr.grad) <= ORACLE


# ---------------------------------------------------------------------------------------------- AdamW
def test_adamw_reference_is_torch_adamw_in_fp64():
    torch.manual_seed(0)
    ps = [torch.randn(1000, dtype=torch.float64), torch.randn(37, 5, dtype=torch.float64), torch.randn(1, dtype=torch.float64)]
    kw = dict(lr=5e-4, weight_decay=1e-2, betas=(0.9, 0.95), eps=1e-8)
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW(ref, **kw)
    mine = [(p.clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    for step in range(1, 5):
        gs = [torch.randn_like(p) * 10.0 ** (step - 2) for p in ps]
        for r, g in zip(ref, gs):
            r.grad = g.clone()
        opt.step()
        mine = [R.adamw_step(p, g, m, v, step, kw["lr"], 0.9, 0.95, kw["eps"], kw["weight_decay"])
                for (p, m, v), g in zip(mine, gs)]
    for r, (p, m, v) in zip(ref, mine):
        st = opt.state[r]
        assert max_rel(p, r) <= 1e-14 and max_rel(m, st["exp_avg"]) <= 1e-14 and max_rel(v, st["exp_avg_sq"]) <= 1e-14


# ---------------------------------------------------------------------------------------------- Muon / NorMuon
def test_muon_reference_is_the_oracle_in_fp64():
    """(a) fp64 R.muon_step == oracle.muon_oracle.muon_step evaluated in fp64, to 1e-12: Muon and NorMuon, Nesterov on and
    off, a wide, a tall and a one-row matrix."""
    from oracle import muon_oracle as MO
    for si, shape in enumerate(((24, 40), (40, 24), (1, 40))):
        for normuon in (False, True):
            for nesterov in (False, True):
                w, g, m = (seeded(10 * si + k, *shape).double() for k in range(3))
                v = (seeded(10 * si + 3, shape[0], 1, kind="rand").abs() + 0.5).double() / max(shape) if normuon else None
                adjust = "rms_norm" if normuon else "spectral_norm"
                mo, vo = m.clone(), None if v is None else v.clone()
                wo = MO.muon_step(w, g, mo, lr=5e-3, mu=0.95, weight_decay=0.01, eps=1e-8, nesterov=nesterov,
                                  adjust=adjust, V=vo, beta2=0.95)
                wn, mn, vn, _ = R.muon_step(w, g, m, v, lr=5e-3, lr_adj=MO.adjusted_lr(5e-3, shape, adjust), mu=0.95,
                                            beta2=0.95, weight_decay=0.01, eps=1e-8, nesterov=nesterov)
                assert max_rel(wn, wo) <= 1e-12 and max_rel(mn, mo) <= 1e-12, (shape, normuon, nesterov)
                assert vn is None or max_rel(vn, vo) <= 1e-12
    assert R.NS_COEFFS == MO.NS_COEFFS


def test_muon_product_orders_are_fp32_products():
    """the three orders and the bf16x3 emulation against the fp64 product: fp32 level (a K = 300 dot product of N(0,1)
    terms: 2e-6 is the bound of tests/test_hip_gemm_split.py); exact on small integers"""
    from tests import _muon_cases as C
    a, b = seeded(1, 37, 300), seeded(2, 300, 41)
    ref = a.double() @ b.double()
    for name, mm in C.ORDERS.items():
        assert max_rel(mm(a, b), ref) <= 2e-6, name
    g = torch.Generator().manual_seed(3)
    a, b = torch.randint(-8, 9, (5, 40), generator=g).float(), torch.randint(-8, 9, (40, 7), generator=g).float()
    for name, mm in C.ORDERS.items():
        assert torch.equal(mm(a, b).double(), a.double() @ b.double()), name


def test_muon_fp32_yardsticks_stay_under_the_ceiling():
    """(b) at every matrix of the GPU cases (tests/_muon_cases.py) the update seen through w = 0, and NorMuon's v, of each
    of the four fp32 evaluations sit under the 1e-5 ceiling the kernels are held to: the ceiling is not one the reference
    side itself would miss."""
    from tests import _muon_cases as C
    worst = 0.0
    for rows, cols, member, nesterov in C.matrices():
        for normuon in (False, True):
            r = C.refs(rows, cols, member, nesterov, normuon, w_zero=True)
            for name, (w, v) in r["cpu"].items():
                e = [C.err(w, r["w64"])] + ([C.err(v, r["v64"])] if normuon else [])
                worst = max([worst] + e)
                assert max(e) <= C.CEILING, ((rows, cols, member, nesterov), normuon, name, e)
    r = C.refs(33, 31, 0, False, True, w_zero=True, v_zero=True)          # the first NorMuon step: v = 0 going in
    for name, (w, v) in r["cpu"].items():
        assert max(C.err(w, r["w64"]), C.err(v, r["v64"])) <= C.CEILING, ("first step", name)
    print(f"largest e_cpu of the update / v over all matrices: {worst:.2e}")


def test_muon_bound_sees_a_wrong_coefficient():
    """(c) a fourth-digit typo in one Newton-Schulz coefficient (2.8769 -> 2.8766) moves the fp64 update by more than ten
    times the ceiling at a small, a mid-sized and the largest shape (1.2e-4 .. 2.2e-4).  A matrix of rank one (1 x 40,
    40 x 1) has a single singular value, which the fifth iteration pulls back towards its fixed point: 3.8e-5 there,
    still above the ceiling (asserted: three times)."""
    from tests import _muon_cases as C
    typo = tuple((2.8766, b, c) if a == 2.8769 else (a, b, c) for a, b, c in R.NS_COEFFS)
    assert typo != R.NS_COEFFS
    for rows, cols, member, nesterov, factor in [(33, 31, 0, False, 10), (64, 96, 0, True, 10), (513, 520, 0, True, 10),
                                                 (1, 40, 0, False, 3), (40, 1, 0, True, 3)]:
        i = C.inputs(rows, cols, member)
        _, o = R.muon_momentum(i["g"].double(), i["m"].double(), C.MU, nesterov)
        moved = C.err(R.newton_schulz(o, C.EPS, coeffs=typo), C.orth(rows, cols, member, nesterov)["x64"])
        print(f"typo moves {rows}x{cols} by {moved:.2e}")
        assert moved > factor * C.CEILING, ((rows, cols), moved)
