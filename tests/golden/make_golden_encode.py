#!/usr/bin/env python3
"""Generates tests/golden/e1_encode.pt by importing the REFERENCE's own ``utils.postprocessing.
convert_cartesian_to_spherical_winds`` and ``utils.mhuaes.mhuaes3`` (both numpy only; under /root/reference) and driving
them as ``utils/file_output.py::_build_dataset_for_samples`` does for the initial state of a forecast file.  That module
itself needs xarray / dask and cannot be imported: its gather loop (``init_data``, :86-108) is restated by
tests/encode_oracle.py::gathered_init.  Run in the build container only.  Only data is stored.

  e1_encode.pt   8x16 and 9x16, B = 2, default names and levels: the recipe and checksum of the seeded raw store rows
                 (tests/encode_oracle.py regenerates them), the sample indices and their store rows, the reference's
                 converted init_data (NaN where an output is not an input) and its dew-point depression."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG                                         # noqa: E402  (puts /root/reference on sys.path)
from utils import postprocessing as PP                           # noqa: E402
from utils.mhuaes import mhuaes3                                 # noqa: E402
from tests import encode_oracle as EO                            # noqa: E402
from tests import forecast_oracle as FO                          # noqa: E402

N_TIME_INPUTS, INTERVAL, BASE, T = 2, 1, 1, 6
INDICES = [3, 0]


def e1_encode():
    cfg = MG.load_cfg()
    levels = list(cfg.features.pressure_levels)
    ins, outs = EO.feature_lists(cfg)
    out = {"numpy": np.__version__, "names": outs, "input_names": ins, "levels": levels, "indices": INDICES,
           "n_time_inputs": N_TIME_INPUTS, "interval_steps": INTERVAL, "base": BASE, "T": T, "cases": {}}
    rows = EO.init_rows(BASE, N_TIME_INPUTS, INTERVAL, INDICES)
    for (H, W, poles, seed) in ((8, 16, False, 801), (9, 16, True, 802)):
        features = EO.store_features(cfg, seed)
        store = EO.raw_store(seed + 10, features, T, H, W)
        lat, lon = FO.grid_deg(H, W, poles, np.float64)
        init = EO.gathered_init(store.numpy(), features, rows, ins, outs)
        gathered_nan = np.isnan(init[0, 0, :, 0, 0])
        PP.convert_cartesian_to_spherical_winds(lat, lon, cfg, init, list(outs))
        assert init.dtype == np.float32 and (np.isnan(init[0, 0, :, 0, 0]) == gathered_nan).all()
        q = init[:, :, PP.get_var_indices("specific_humidity", outs)]
        tt = init[:, :, PP.get_var_indices("temperature", outs)]
        ps = (np.asarray(levels) * 100)[:, None, None]               # integer hPa * 100, as the writer builds it
        assert ps.dtype.kind == "i" and q.dtype == np.float32
        dew = mhuaes3(q, tt, ps).astype("float32")
        out["cases"][f"{H}x{W}"] = {
            "H": H, "W": W, "poles": poles, "seed": seed, "features": features, "rows": rows, "chk": MG.chk(store),
            "init": torch.from_numpy(init.copy()), "dew": torch.from_numpy(dew.copy()),
            "nan_channels": [outs[i] for i in np.where(gathered_nan)[0]]}
    path = os.path.join(HERE, "e1_encode.pt")
    torch.save(out, path)
    print("wrote e1_encode.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    e1_encode()
