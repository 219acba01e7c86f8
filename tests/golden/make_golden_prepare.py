#!/usr/bin/env python3
"""Generates tests/golden/p1_prepare.pt by importing the REFERENCE's own functions (as make_golden_forecast.py does;
run in the build container only).  Only data is stored: seeds and checksums of the inputs (tests/prepare_oracle.py
regenerates them) and the reference's outputs.

  winds   utils.postprocessing.compute_cartesian_wind - the formula of scripts/preprocess_dataset.py's function of that
          name in plain numpy, its ``w`` being omega - on float32 fields and float64 grids, 9x16 with poles and 8x15
          without, 3 levels, T = 2: the six float32 outputs
  toa     data.forcings.toa_radiation.toa_radiation_stats: 9 times 1 h apart on the 9x16 grid, strides (1, 1, 1) and
          (2, 2, 3): (mean, std), and the maximum of the radiation over the case (the scale of the tests' bound)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG                                         # noqa: E402,F401  (puts the reference on sys.path)
from utils import postprocessing as PP                           # noqa: E402
import data.forcings.toa_radiation  # noqa: E402
TR = sys.modules["data.forcings.toa_radiation"]  # (the package re-exports a function of the module's name)
from tests import prepare_oracle as PO                           # noqa: E402

TOA_T0 = "2021-03-19T20:00"
TOA_STRIDES = [(1, 1, 1), (2, 2, 3)]


def main():
    out = {"numpy": np.__version__, "levels": PO.LEVELS, "winds": {}, "toa": {}}
    for n, (H, W, poles) in enumerate(PO.WIND_GRIDS):
        seed = 701 + n
        f = PO.wind_fields(seed, PO.WIND_T, len(PO.LEVELS), H, W)
        lat, lon = PO.grid_deg(H, W, poles)
        got = PP.compute_cartesian_wind(lat[:, None], lon[None, :], np.asarray(PO.LEVELS), f["t"], f["u"], f["v"], f["w"],
                                        f["u10"], f["v10"])
        assert all(a.dtype == np.float64 for a in got)
        rec = {"H": H, "W": W, "poles": poles, "seed": seed,
               "chk": [float(sum(np.abs(a.astype(np.float64)).sum() for a in f.values()))]}
        for key, a in zip(("x", "y", "z", "x10", "y10", "z10"), got):
            rec[key] = torch.from_numpy(a.astype(np.float32))
        out["winds"][f"{H}x{W}"] = rec
    H, W, poles = PO.WIND_GRIDS[0]
    lat, lon = PO.grid_deg(H, W, poles)
    times = np.datetime64(TOA_T0, "us") + np.arange(9) * np.timedelta64(1, "h")
    out["toa"] = {"t0": TOA_T0, "n_times": 9, "grid": [H, W, poles], "cases": []}
    for (ts, ls, lo) in TOA_STRIDES:
        mean, std = TR.toa_radiation_stats(times, lat, lon, ts, ls, lo)
        # the scale of the bound: the largest value of the fields the statistics are taken over (same arguments as :221-230)
        lat_rad = (lat[::ls].reshape(-1, 1) * np.pi / 180).astype(np.float32)
        lon_deg = lon[::lo].reshape(1, -1).astype(np.float32)
        peak = max(float(TR.toa_radiation_1h(lat_rad, lon_deg, t.astype(np.float64)).max()) for t in times[::ts])
        out["toa"]["cases"].append({"strides": [ts, ls, lo], "mean": mean, "std": std, "max": peak})
    path = os.path.join(HERE, "p1_prepare.pt")
    torch.save(out, path)
    print("wrote p1_prepare.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
