"""Decode error of the 16-bit packed store per normalisation kind, from the CPU restatement (tests/pack_oracle.py): the
table of DESIGN.md "The packed store".  No GPU.  For each kind 200 synthetic planes of 4,096 values are packed and
decoded, both copies are normalised the way the feed normalises them (float32), and the largest difference is printed
in physical and in normalised units, next to the bound of the plane it occurred in.

    python tools/pack_error_table.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pack_oracle as PK   # noqa: E402

f32 = np.float32
Q_MIN, Q_MAX, EPS_Q = f32(1e-8), f32(0.03), f32(1e-12)


def zscore(mean, std):
    return lambda x: ((x - f32(mean)) / f32(std)).astype(f32)


def humidity(x):
    lmin, lmax = np.log(Q_MIN), np.log(Q_MAX)
    return ((np.log(np.minimum(np.maximum(x, f32(0)), Q_MAX) + EPS_Q).astype(f32) - lmin) / (lmax - lmin)).astype(f32)


def precip_plane(r):
    return np.where(r.random(4096) < 0.6, 0.0, np.exp(r.uniform(np.log(1e-7), np.log(0.2), 4096)))


# name, plane generator, normalisation, packing domain
ROWS = [
    ("z-score: temperature, 100 K wide (std 20 K)", lambda r: 230 + 100 * r.random(4096), zscore(280, 20), PK.LINEAR),
    ("z-score: geopotential, 3e4 wide at 5e5 (std 3e3)", lambda r: 4.85e5 + 3e4 * r.random(4096), zscore(5e5, 3e3),
     PK.LINEAR),
    ("humidity 1e-8 .. 3e-2, linear domain", lambda r: np.exp(r.uniform(np.log(1e-8), np.log(3e-2), 4096)), humidity,
     PK.LINEAR),
    ("humidity 1e-8 .. 3e-2, log domain (log_packed)", lambda r: np.exp(r.uniform(np.log(1e-8), np.log(3e-2), 4096)),
     humidity, PK.LOG),
    ("precipitation 0 .. 0.2 m, linear domain", precip_plane, PK.normalise_precip, PK.LINEAR),
    ("precipitation 0 .. 0.2 m, log domain (default)", precip_plane, PK.normalise_precip, PK.LOG),
]


def main():
    print("| plane | step | worst error, physical | worst error, normalised |")
    print("|---|---|---|---|")
    for k, (name, gen, norm, domain) in enumerate(ROWS):
        rng = np.random.default_rng(100 + k)
        phys = normd = step = 0.0
        for _ in range(200):
            x = gen(rng).astype(f32)
            codes, lo, s = PK.pack_plane(x, domain)
            back = PK.unpack_plane(codes, lo, s, domain)
            phys = max(phys, float(np.abs(back.astype(np.float64) - x).max()))
            normd = max(normd, float(np.abs(norm(back).astype(np.float64) - norm(x)).max()))
            step = max(step, float(s))
        unit = "of log(x + 1e-6)" if domain == PK.LOG else ""
        print(f"| {name} | {step:.3g} {unit} | {phys:.3g} | {normd:.3g} |")


if __name__ == "__main__":
    main()
