"""AMSE loss (sht.hip) timing: HIP-event times of the table build and of one value + gradient call, with the algorithmic
FLOPs of the four GEMM stages (direct DFT, Legendre analysis, adjoint Legendre, adjoint DFT) and the f32 MFMA share they
imply.  Grids of DESIGN.md section 4.9: 721 x 1440 with B=1, C=97 and 33 x 64 with B=32, C=97.  Needs the MI355X.

    python tools/amse_bench.py [--iters N]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_PEAK = 157.3e12      # MI355X, v_mfma_f32_16x16x4_f32 (MI355X_MICROARCH: 155 TF measured)


def flops(B, C, H, W):
    N, M = B * C, H - 1
    tri = M * (M + 1) // 2
    return {
        "dft_fwd": 2.0 * (2 * N * H) * W * (2 * M),        # pred + target, Re + Im
        "legendre_fwd": 2.0 * (4 * N) * tri * H,
        "legendre_adj": 2.0 * (2 * N) * tri * H,
        "dft_adj": 2.0 * (N * H) * (2 * M) * W,
    }


def run(B, C, H, W, iters):
    from paradis_model_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(B, C, H, W, device=dev, generator=g).requires_grad_(True)
    t = torch.randn(B, C, H, W, device=dev, generator=g)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops._AMSE_TABLES.clear()
    e0.record()
    leg, tw = ops.amse_tables(H, W, dev)
    e1.record()
    torch.cuda.synchronize()
    table_ms = e0.elapsed_time(e1)

    def one(want_grad):
        return torch.ops.paradis.amse_loss(p.detach(), t, leg, tw, want_grad)

    for _ in range(2):
        one(True)
    out = {}
    for name, wg in (("fwd", False), ("fwd_bwd", True)):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            one(wg)
        e1.record()
        torch.cuda.synchronize()
        out[name + "_ms"] = e0.elapsed_time(e1) / iters
    f = flops(B, C, H, W)
    fwd = f["dft_fwd"] + f["legendre_fwd"]
    tot = fwd + f["legendre_adj"] + f["dft_adj"]
    res = {"grid": f"{H}x{W}", "B": B, "C": C, "table_build_ms": round(table_ms, 3),
           "table_MB": round(leg.numel() * 4 / 2 ** 20, 1),
           "fwd_ms": round(out["fwd_ms"], 3), "fwd_bwd_ms": round(out["fwd_bwd_ms"], 3),
           "gemm_TFLOP_fwd": round(fwd / 1e12, 4), "gemm_TFLOP_fwd_bwd": round(tot / 1e12, 4),
           "TFLOPs_fwd": round(fwd / out["fwd_ms"] / 1e9, 2), "TFLOPs_fwd_bwd": round(tot / out["fwd_bwd_ms"] / 1e9, 2)}
    res["mfma_util_fwd_bwd"] = round(res["TFLOPs_fwd_bwd"] * 1e12 / F32_MFMA_PEAK, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amse_bench.py needs the GPU")
    for B, C, H, W in ((1, 97, 721, 1440), (32, 97, 33, 64)):
        print(json.dumps(run(B, C, H, W, a.iters)), flush=True)


if __name__ == "__main__":
    main()
