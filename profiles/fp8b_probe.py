"""Block-scaled FP8 (e4m3 codes, one fp32 scale per 16-row group and 128 columns on the device) measurements on one MI355X; the
shared pieces come from w4a16_probe.py.

  python profiles/fp8b_probe.py gemm [--reps 40]
      the 70B verify GEMMs at M = 8: per-row (ssd_gemm_fp8) and block-scaled (ssd_gemm_fp8b) alternating twice in the same process
      (fp8, fp8b, fp8, fp8b: the gap between the two fp8 passes is the spread a ratio is read against; the margin is that spread
      doubled) on the SAME codes, each launch shape over 8 distinct weight copies (> the 256 MiB Infinity Cache), HIP-event time
      per launch and the fraction of 8 TB/s on the bytes each actually streams; a summary line per matrix; then the two prefill
      routes at M = 32 / 64 / 128 (block-scaled GEMM vs ssd_fp8b_dequant_frag + ssd_gemm_pf).
  python profiles/fp8b_probe.py sweep [--reps 10] [--models 70b,qwen3-32b]
      every explicit decomposition (ssd_gemm_fp8b_cfg) of the four matrices at M = 8: the four fastest per matrix and the default.
  python profiles/fp8b_probe.py step [--block] [--steps 20 --warmup 5]
      the c4 workload exactly as w4a16_probe.py builds it with quantization="fp8"; with --block every synthetic linear goes
      through quantize_fp8_block as it reaches the decoder (there is no on-load switch for block scales: the probe hands the
      decoder the tuple a block-scaled checkpoint would), so the target runs on ssd_gemm_fp8b.
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

HBM = P.HBM
PASSES = ("fp8", "fp8b", "fp8", "fp8b")
COPIES = 8


def _fp8(N, K, dev):
    """codes (no NaN codes), per-row scales, group table"""
    q = torch.randint(0, 256, (N * K,), dtype=torch.uint8, device=dev)
    q[(q & 0x7f) == 0x7f] = 0x3c
    s = torch.rand(N, device=dev) * 1e-3 + 1e-4
    sb = torch.rand(N // 16, -(-K // 128), device=dev) * 1e-3 + 1e-4
    return q, s, sb


def fp8_bytes(N, K):
    return N * K + 4 * N


def fp8b_bytes(N, K):
    return N * K + 4 * (N // 16) * -(-K // 128)


def gemm(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import fp8b_ops as F8B
    dev = torch.device("cuda", 0)
    shapes = P._shapes(P.MODELS["70b"])
    M = 8
    for kind, (N, K, epi) in shapes.items():
        x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
        y = torch.empty(max(M, 16) * N, dtype=torch.bfloat16, device=dev)
        ldy = 0 if epi == H.EPI_SILU_FRAG else N
        ws = [_fp8(N, K, dev) for _ in range(COPIES)]
        got = {"fp8": [], "fp8b": []}
        for i, dtype in enumerate(PASSES):
            nbytes = fp8b_bytes(N, K) if dtype == "fp8b" else fp8_bytes(N, K)

            def run():
                for w in ws:
                    if dtype == "fp8b":
                        F8B.gemm_fp8b(x, w[0], w[2], y, M, N, K, ldy, epi)
                    else:
                        Q.gemm_fp8(x, w[0], w[1], y, M, N, K, ldy, epi)
            us = statistics.median(P._time(run, args.reps) / COPIES for _ in range(3))
            got[dtype].append(us)
            print(json.dumps({"probe": "verify_gemm", "M": M, "kind": kind, "N": N, "K": K, "dtype": dtype, "pass": i, "us": round(us, 2),
                              "bytes": nbytes, "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
        row, blk = sum(got["fp8"]) / 2, sum(got["fp8b"]) / 2
        spread = abs(got["fp8"][0] - got["fp8"][1]) / row
        print(json.dumps({"probe": "verify_gemm_summary", "kind": kind, "fp8_us": round(row, 2), "fp8b_us": round(blk, 2),
                          "fp8b_over_fp8": round(blk / row, 4), "fp8_spread": round(spread, 4), "margin": round(2 * spread, 4),
                          "within_margin": blk / row <= 1 + 2 * spread}), flush=True)
        del ws
        torch.cuda.empty_cache()
    for M in (32, 64, 128):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(M * N, dtype=torch.bfloat16, device=dev)
            q, s, sb = _fp8(N, K, dev)
            deq = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
            wsp = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=dev)
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            t_row = P._time(lambda: Q.gemm_fp8(x, q, s, y, M, N, K, ldy, epi), args.reps)
            t_blk = P._time(lambda: F8B.gemm_fp8b(x, q, sb, y, M, N, K, ldy, epi), args.reps)
            t_deq = P._time(lambda: (F8B.fp8b_dequant_frag(q, sb, deq, N, K), H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi)),
                            args.reps)
            print(json.dumps({"probe": "prefill_chunk", "M": M, "kind": kind, "fp8_gemm_us": round(t_row, 2),
                              "fp8b_gemm_us": round(t_blk, 2), "dequant_plus_gemm_pf_us": round(t_deq, 2)}), flush=True)
            del q, s, sb, deq, wsp
            torch.cuda.empty_cache()


def sweep(args):
    """Every explicit decomposition of ssd_gemm_fp8b_cfg at M = 8 (8 weight copies per launch shape)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import fp8b_ops as F8B
    dev = torch.device("cuda", 0)
    M = 8
    for model in args.models.split(","):
        for kind, (N, K, epi) in P._shapes(P.MODELS[model]).items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(16 * N, dtype=torch.bfloat16, device=dev)
            ws = [_fp8(N, K, dev) for _ in range(COPIES)]
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            nbytes = fp8b_bytes(N, K)
            res = []
            for nt in ((2, 4) if epi == H.EPI_SILU_FRAG else (1, 2, 4)):
                if (N // 16) % nt:
                    continue
                for deep in (0, 1):
                    for waves in (2, 4, 8):
                        for tpw in (1, 2, 4):
                            cfg = (nt | (deep << 8), waves | (tpw << 8))

                            def run():
                                for w in ws:
                                    F8B.gemm_fp8b(x, w[0], w[2], y, M, N, K, ldy, epi, cfg=cfg)
                            res.append((P._time(run, args.reps) / COPIES, nt, deep, waves, tpw))

            def run_default():
                for w in ws:
                    F8B.gemm_fp8b(x, w[0], w[2], y, M, N, K, ldy, epi)
            d_us = statistics.median(P._time(run_default, args.reps) / COPIES for _ in range(3))
            res.sort()
            for us, nt, deep, waves, tpw in res[:4]:
                print(json.dumps({"probe": "sweep", "model": model, "kind": kind, "N": N, "K": K, "nt": nt, "deep": deep, "waves": waves,
                                  "tpw": tpw, "us": round(us, 2), "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
            print(json.dumps({"probe": "sweep_default", "model": model, "kind": kind, "us": round(d_us, 2),
                              "frac_8TBs": round(nbytes / (d_us * 1e-6) / HBM, 4)}), flush=True)
            del ws
            torch.cuda.empty_cache()


def step(args):
    args.quant = "fp8"
    if args.block:
        from ssd_amd import quant
        from ssd_amd.model import HipDecoder
        HipDecoder._quantize_on_load = lambda self, w: quant.quantize_fp8_block(w)      # bf16 linears become block-scaled on load
    print(json.dumps({"probe": "mode", "quant": "fp8", "block_scaled": bool(args.block), "reading": "single"}), flush=True)
    P.step(args)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gemm", "sweep", "step"])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--block", action="store_true")
    ap.add_argument("--models", default="70b,qwen3-32b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"gemm": gemm, "sweep": sweep, "step": step}[a.mode](a)
