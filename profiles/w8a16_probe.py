"""W8A16 (int8 codes, one bf16 scale per row and 128 columns) measurements on one MI355X; the shared pieces come from w4a16_probe.py.

  python profiles/w8a16_probe.py gemm [--reps 40]
      the four 70B verify GEMMs at M = 8: ssd_gemm_fp8 and ssd_gemm_w8a16 alternating twice in the same process (fp8, w8a16, fp8,
      w8a16: the gap between the two fp8 passes is the spread a ratio is read against; the margin is that spread doubled plus the
      byte difference), each launch shape over 8 distinct weight copies (> the 256 MiB Infinity Cache), HIP-event time per launch and
      the fraction of 8 TB/s on the bytes each actually streams; a summary line per matrix; then both kernels at M = 32 / 64 / 128.
  python profiles/w8a16_probe.py step --quant w8a16|fp8 [--steps 20 --warmup 5]
      the c4 workload exactly as w4a16_probe.py builds it.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import w4a16_probe as P  # noqa: E402

PASSES = ("fp8", "w8a16", "fp8", "w8a16")
COPIES = 8


def _weights(N, K, dev):
    """random bytes that are valid for both kernels (no fp8 NaN codes), fp8 row scales, w8 group scales"""
    q = torch.randint(0, 256, (N * K,), dtype=torch.uint8, device=dev)
    q[(q & 0x7f) == 0x7f] = 0x3c
    return q, torch.rand(N, device=dev) * 1e-3 + 1e-4, (torch.rand(N * K // 128, device=dev) * 4e-4 + 1e-4).to(torch.bfloat16)


def nbytes(dtype, N, K):
    return N * K + (4 * N if dtype == "fp8" else 2 * N * K // 128)


def _call(dtype, x, w, y, M, N, K, ldy, epi):
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import w8_ops as W8
    if dtype == "fp8":
        Q.gemm_fp8(x, w[0], w[1], y, M, N, K, ldy, epi)
    else:
        W8.gemm_w8a16(x, w[0], w[2], y, M, N, K, ldy, epi)


def gemm(args):
    from ssd_amd.hip import ops as H
    dev = torch.device("cuda", 0)
    shapes = P._shapes(P.MODELS["70b"])
    for M in (8, 32, 64, 128):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(max(M, 16) * N, dtype=torch.bfloat16, device=dev)
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            ws = [_weights(N, K, dev) for _ in range(COPIES)]
            got = {"fp8": [], "w8a16": []}
            for i, dtype in enumerate(PASSES):
                def run():
                    for w in ws:
                        _call(dtype, x, w, y, M, N, K, ldy, epi)
                us = statistics.median(P._time(run, args.reps) / COPIES for _ in range(3))
                got[dtype].append(us)
                b = nbytes(dtype, N, K)
                print(json.dumps({"probe": "gemm", "M": M, "kind": kind, "N": N, "K": K, "dtype": dtype, "pass": i, "us": round(us, 2),
                                  "bytes": b, "frac_8TBs": round(b / (us * 1e-6) / P.HBM, 4)}), flush=True)
            f8, w8 = sum(got["fp8"]) / 2, sum(got["w8a16"]) / 2
            spread = abs(got["fp8"][0] - got["fp8"][1]) / f8
            extra = nbytes("w8a16", N, K) / nbytes("fp8", N, K) - 1
            print(json.dumps({"probe": "gemm_summary", "M": M, "kind": kind, "fp8_us": round(f8, 2), "w8a16_us": round(w8, 2),
                              "w8a16_over_fp8": round(w8 / f8, 4), "fp8_spread": round(spread, 4), "byte_difference": round(extra, 4),
                              "margin": round(2 * spread + extra, 4), "within_margin": w8 / f8 <= 1 + 2 * spread + extra}), flush=True)
            del ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gemm", "step"])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--quant", default="w8a16", choices=["fp8", "w8a16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"gemm": gemm, "step": P.step}[a.mode](a)
