#!/usr/bin/env python3
"""Generates tests/golden/v1_val.pt by importing the REFERENCE's own ParadisLoss (utils/loss.py), its
utils/normalization.py and its model under /root/reference, and driving them through a restated ``validation_step`` and
``_get_report_rmse`` (trainer.py:652-708, 291-315; Lightning is not importable, as for c2_rollout and f5_forecast).
Run in the build container only.  Only data is stored: recipes and checksums of the seeded inputs
(tests/val_oracle.py regenerates them), the branch each report feature took, and the reference's numbers.

  single   8x16 and 9x16 (poles), B = 2, one state, 97 channels: loss, per_channel_loss weighted / unweighted and the
           report RMSE of five report features (a humidity level, total_precipitation_6hr, two z-score, one duplicate)
           for custom normalisation on / off x {reversed_huber, mse} x latitude weights on / off
  rollout  variant "a" with g4_model_a.pt["state"], 16x32, B = 2, S = 3, custom norms on: the per-step rows, the
           logged step means, and per number the L1 norm of the fp64 gradient with respect to that step's prediction
           plus max|y| of the step (the test's first-order bound)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG                                         # noqa: E402  (puts /root/reference on sys.path)
from utils.normalization import denormalize_humidity, denormalize_precipitation      # noqa: E402
from tests import forecast_oracle as FO                          # noqa: E402
from tests import val_oracle as VO                               # noqa: E402


def report_rmse(loss_fn, report_features, report_ind, report_std, custom_norms, q_min, q_max, output_data, pred_data,
                branches=None):
    """trainer.py:291-315 line by line; ``branches`` records the branch each feature takes"""
    lat_weights = loss_fn.lat_weights.view(1, 1, -1, 1).to(output_data.dtype)
    errors = torch.empty(len(report_ind), dtype=output_data.dtype)
    for i, ind in enumerate(report_ind):
        if custom_norms and "specific_humidity" in report_features[i]:
            o_data = denormalize_humidity(output_data[:, ind], q_min, q_max)
            p_data = denormalize_humidity(pred_data[:, ind], q_min, q_max)
            errors[i] = torch.mean((o_data - p_data) ** 2 * lat_weights)
            branch = "humidity"
        elif custom_norms and "precipitation" in report_features[i]:
            o_data = denormalize_precipitation(output_data[:, ind])
            p_data = denormalize_precipitation(pred_data[:, ind])
            errors[i] = torch.mean((o_data - p_data) ** 2 * lat_weights)
            branch = "precipitation"
        else:
            errors[i] = torch.mean(((output_data[:, ind] - pred_data[:, ind]) * report_std[i]) ** 2 * lat_weights)
            branch = "zscore"
        if branches is not None:
            branches.append(branch)
    return torch.sqrt(errors)


def score_row(loss_fn, out, tgt, rep):
    """what validation_step (and the per-channel logging of training_step) evaluate for one step"""
    return torch.cat([loss_fn(out, tgt).reshape(1), loss_fn.per_channel_loss(out, tgt, weighted=True),
                      loss_fn.per_channel_loss(out, tgt, weighted=False), rep(out, tgt)])


def make_loss(cfg, lat_deg, kind, latw):
    cfg.training.loss_function.type = kind
    cfg.training.loss_function.lat_weights = latw
    return MG.loss_pieces(cfg, lat_deg)


def single(names):
    cases = {}
    feats = VO.SINGLE_REPORTS
    ind = torch.tensor([names.index(f) for f in feats], dtype=torch.long)      # dyn_input_features.index(feature)
    std = VO.report_std(names, feats)
    q_min, q_max = torch.tensor(FO.Q_MIN), torch.tensor(FO.Q_MAX)
    for (H, W, poles, seed) in ((8, 16, False, 701), (9, 16, True, 702)):
        lat_deg, _, _ = MG.grid(H, W, poles)
        pred, tgt = VO.single_state(seed, names, 2, H, W)
        rec = {"H": H, "W": W, "poles": poles, "seed": seed, "chk": MG.chk(pred) + MG.chk(tgt), "lat_deg": lat_deg,
               "rows": {}}
        for custom in (True, False):
            br = []
            report_rmse(make_loss(MG.load_cfg(), lat_deg, "mse", True)[0], feats, ind, std, custom, q_min, q_max, pred,
                        tgt, br)
            rec[f"branches_custom{int(custom)}"] = br
            for kind in ("reversed_huber", "mse"):
                for latw in (True, False):
                    cfg = MG.load_cfg()
                    fn, _, order = make_loss(cfg, lat_deg, kind, latw)
                    assert order == names
                    with torch.no_grad():
                        rec["rows"][(custom, kind, latw)] = score_row(
                            fn, pred, tgt, lambda o, t: report_rmse(fn, feats, ind, std, custom, q_min, q_max, o, t))
                    rec["delta"] = float(cfg.training.loss_function.delta_loss)
        cases[f"{H}x{W}"] = rec
    return {"features": feats, "indices": ind.tolist(), "std": std, "cases": cases}


def rollout(names):
    cfg, model, lat_deg, lg, og = MG.build_model("a")
    g4 = torch.load(os.path.join(HERE, "g4_model_a.pt"), weights_only=False)
    model.load_state_dict(g4["state"])
    model.eval()
    fn, _, order = MG.loss_pieces(cfg, lat_deg)
    assert order == names
    feats = VO.ROLLOUT_REPORTS
    ind = torch.tensor([names.index(f) for f in feats], dtype=torch.long)
    std = VO.report_std(names, feats)
    q_min, q_max = torch.tensor(FO.Q_MIN), torch.tensor(FO.Q_MAX)
    H, W = lg.shape
    B, S, ncom = 2, 3, 83
    inp = MG.seeded(477, B, 1, 166, H, W)
    true = FO.normalised_state(478, names, B, S, len(names), H, W)
    forc = MG.seeded(479, B, S, H, W, 10, kind="rand")
    const = MG.seeded(480, B, 1, H, W, 10)
    # validation_step, trainer.py:655-686
    constants = const[:, :1].permute(0, 1, 4, 2, 3)
    forcings = forc.permute(0, 1, 4, 2, 3)
    cur, val_loss, report_loss, rows, outs = inp, 0.0, 0.0, [], []
    br = []
    with torch.no_grad():
        for step in range(S):
            mi = torch.cat([cur, forcings[:, step].unsqueeze(1), constants], dim=2).squeeze(1)
            y = model(mi)
            loss = fn(y, true[:, step])
            rep = report_rmse(fn, feats, ind, std, True, q_min, q_max, y, true[:, step], br if step == 0 else None)
            report_loss = report_loss + rep
            val_loss = val_loss + loss
            rows.append(score_row(fn, y, true[:, step], lambda o, t: rep))
            assert float(rows[-1][0]) == float(loss)
            outs.append(y)
            cur = torch.cat([mi[:, ncom:2 * ncom], y[:, :ncom]], dim=1).unsqueeze(1)
    # the fp64 gradient of every number of a step with respect to that step's prediction: L1 norms
    fn64 = MG.loss_pieces(cfg, lat_deg)[0].double()
    fn64.lat_weights = fn64.lat_weights.double()
    n = rows[0].numel()
    l1 = torch.zeros(S, n, dtype=torch.float64)
    for step in range(S):
        y = outs[step].double().requires_grad_(True)
        r64 = score_row(fn64, y, true[:, step].double(),
                        lambda o, t: report_rmse(fn64, feats, ind, std.double(), True, q_min.double(), q_max.double(), o, t))
        assert float((r64.detach() - rows[step].double()).abs().max() / rows[step].abs().max()) < 1e-5
        for i in range(n):
            (g,) = torch.autograd.grad(r64[i], y, retain_graph=True)
            l1[step, i] = g.abs().sum()
    return {"variant": "a", "state_from": "g4_model_a.pt", "seeds": [477, 478, 479, 480], "B": B, "S": S,
            "chk": MG.chk(inp) + MG.chk(true) + MG.chk(forc) + MG.chk(const), "features": feats,
            "indices": ind.tolist(), "branches": br, "std": std, "rows": torch.stack(rows), "grad_l1": l1,
            "ymax": torch.tensor([float(o.abs().max()) for o in outs], dtype=torch.float64),
            "val_loss": (val_loss / S).clone(), "reports": (report_loss / S).clone(),
            "loss_kind": cfg.training.loss_function.type, "lat_weights": bool(cfg.training.loss_function.lat_weights),
            "delta": float(cfg.training.loss_function.delta_loss)}


if __name__ == "__main__":
    torch.set_num_threads(8)
    import make_golden_forecast as MF                            # noqa: E402
    _, names, _ = MF.names_levels()
    out = {"names": names, "stats_seed": 501, "q_min": FO.Q_MIN, "q_max": FO.Q_MAX, "single": single(names),
           "rollout": rollout(names)}
    path = os.path.join(HERE, "v1_val.pt")
    torch.save(out, path)
    print("wrote v1_val.pt", os.path.getsize(path), "bytes")
