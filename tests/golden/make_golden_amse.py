#!/usr/bin/env python3
"""Golden vectors of the AMSE loss (g8_amse.pt) from the *reference's own* utils/amse_loss.py and utils/loss.py, imported
unmodified (the PSD and coherence loops, the eps values, the clamp, the NaN fallback and ParadisLoss' "x feature weights
then mean" are therefore the reference's code).  torch_harmonics is not installed: the restated RealSHT of
tests/amse_oracle.py is installed in its place as a stub module.

Run in the build container only (the reference tree does not exist on the GPU box):
    python tests/golden/make_golden_amse.py [reference root, default /root/reference]
Grids 9x16 and 33x64; two regimes: independent fields, and p = t + 0.01 * noise.  Stored: seeds and input checksums
(the tests/_util.seeded recipe), loss values, per_channel_loss, feature weights, and sub-sampled gradients.
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

import amse_oracle as O  # noqa: E402
from _util import chk, seeded  # noqa: E402

_th = types.ModuleType("torch_harmonics")
_th.RealSHT = O.RealSHT
sys.modules["torch_harmonics"] = _th

from utils.loss import ParadisLoss  # noqa: E402

B, C = 2, 3
LEVELS = [500.0, 850.0]
GRIDS = [(9, 16, 11), (33, 64, 12)]
GRAD_STRIDE = 7


def inputs(H, W, seed, regime):
    t = seeded(seed, B, C, H, W)
    if regime == "independent":
        p = seeded(seed + 100, B, C, H, W)
    else:
        p = t + 0.01 * seeded(seed + 200, B, C, H, W)
    return p, t


def main():
    torch.set_grad_enabled(True)
    out = {"B": B, "C": C, "levels": LEVELS, "grad_stride": GRAD_STRIDE, "cases": []}
    vw = torch.tensor([1.0, 0.5, 2.0])
    for H, W, seed in GRIDS:
        lat = torch.linspace(-90.0, 90.0, H)
        loss = ParadisLoss("amse", lat, torch.tensor(LEVELS), num_features=C, num_surface_vars=1,
                           var_loss_weights=vw, output_name_order=["t_h0", "t_h1", "msl"], apply_latitude_weights=True)
        assert loss.apply_latitude_weights is False
        for regime in ("independent", "near"):
            p, t = inputs(H, W, seed, regime)
            pr = p.clone().requires_grad_(True)
            val = loss(pr, t)
            val.backward()
            amse = loss.loss_fn(p, t)
            pcl = loss.per_channel_loss(p, t, weighted=True)
            out["cases"].append({
                "H": H, "W": W, "seed": seed, "regime": regime, "chk": chk(p) + chk(t),
                "feature_weights": loss.feature_weights.clone(),
                "loss": float(val), "amse": float(amse), "per_channel": pcl.detach().clone(),
                "grad_sub": pr.grad.reshape(-1)[::GRAD_STRIDE].clone(), "grad_norm": float(pr.grad.norm()),
            })
            print(f"{H}x{W} {regime}: loss {float(val):.6e} amse {float(amse):.6e}")
    torch.save(out, os.path.join(HERE, "g8_amse.pt"))


if __name__ == "__main__":
    main()
