"""MXFP4 (e2m1 codes, e8m0 scale per 32 columns) target measurements on one MI355X; the shared pieces come from w4a16_probe.py.

  python profiles/mxfp4_probe.py gemm [--reps 40]
      the 70B verify GEMMs at M = 8: fp8 (ssd_gemm_fp8), w4a16 (ssd_gemm_w4a16) and mxfp4 (ssd_gemm_mxfp4) in the same process, the two
      4-bit kernels alternating twice (w4a16, mxfp4, w4a16, mxfp4: the gap between the two w4a16 passes is the spread a ratio is read
      against), each launch shape over 8 distinct weight copies (> the 256 MiB Infinity Cache), HIP-event time per launch and the
      fraction of 8 TB/s on the bytes each actually streams; then the two prefill routes at M = 32 / 64 / 128 (mxfp4 GEMM vs
      dequantize + ssd_gemm_pf), which set HipDecoder.MX4_DIRECT_MAX_T.  Run it under `rocprofv3 --kernel-trace --stats` for the
      kernel-level table.
  python profiles/mxfp4_probe.py sweep [--reps 10]
      every explicit decomposition (ssd_gemm_mxfp4_cfg) of the four matrices of the 1B, 8B, 70B and Qwen3-32B at M = 8: the four
      fastest per matrix and the default.
  python profiles/mxfp4_probe.py step --quant {none,fp8,w4a16,mxfp4} [--steps 20 --warmup 5]
      the c4 workload exactly as w4a16_probe.py builds it, plus the quantization keyword: TTFT p50 at 128 and 2048 prompt tokens, ms
      per step and the accepted length.
  python profiles/mxfp4_probe.py ktable --db OUT/mxfp4_results.db
      (no GPU) the per-matrix M = 8 kernel times of a `gemm` run traced with `rocprofv3 --kernel-trace --stats -o mxfp4`: the GEMM
      dispatches in launch order come in runs of 41 x 8 per (matrix, pass), in the order the probe launches them; prints CSV.
  python profiles/mxfp4_probe.py qerr
      (no GPU) relative Frobenius error of mxfp4, w4a16 and fp8 on N(0, 0.02) matrices and on correlated-pair weights.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import w4a16_probe as P  # noqa: E402

HBM = P.HBM
PASSES = ("fp8", "w4a16", "mxfp4", "w4a16", "mxfp4")


def _mx4(N, K, dev):
    q = torch.randint(0, 256, (N * K // 2,), dtype=torch.uint8, device=dev)
    s = torch.randint(117, 124, (N * K // 32,), dtype=torch.uint8, device=dev)
    return q, s


def mx4_bytes(N, K):
    return N * K // 2 + N * K // 32


def gemm(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import w4_ops as W4
    from ssd_amd.hip import mx4_ops as MX4
    dev = torch.device("cuda", 0)
    shapes = P._shapes(P.MODELS["70b"])
    COPIES, M = 8, 8
    for kind, (N, K, epi) in shapes.items():
        x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
        y = torch.empty(max(M, 16) * N, dtype=torch.bfloat16, device=dev)
        s8 = torch.rand(N, device=dev) * 1e-3
        ldy = 0 if epi == H.EPI_SILU_FRAG else N
        for i, dtype in enumerate(PASSES):
            if dtype == "fp8":
                ws = [torch.randint(0, 0x7e, (N * K,), dtype=torch.uint8, device=dev) for _ in range(COPIES)]
                nbytes = N * K + 4 * N
            elif dtype == "w4a16":
                ws = [P._w4(N, K, dev) for _ in range(COPIES)]
                nbytes = P.w4_bytes(N, K)
            else:
                ws = [_mx4(N, K, dev) for _ in range(COPIES)]
                nbytes = mx4_bytes(N, K)

            def run():
                for w in ws:
                    if dtype == "fp8":
                        Q.gemm_fp8(x, w, s8, y, M, N, K, ldy, epi)
                    elif dtype == "w4a16":
                        W4.gemm_w4a16(x, w[0], w[1], y, M, N, K, ldy, epi)
                    else:
                        MX4.gemm_mxfp4(x, w[0], w[1], y, M, N, K, ldy, epi)
            us = P._time(run, args.reps) / COPIES
            print(json.dumps({"probe": "verify_gemm", "M": M, "kind": kind, "N": N, "K": K, "dtype": dtype, "pass": i, "us": round(us, 2),
                              "bytes": nbytes, "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
            del ws
            torch.cuda.empty_cache()
    for M in (32, 64, 128):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(M * N, dtype=torch.bfloat16, device=dev)
            q, s = _mx4(N, K, dev)
            deq = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
            wsp = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=dev)
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            t_mx = P._time(lambda: MX4.gemm_mxfp4(x, q, s, y, M, N, K, ldy, epi), args.reps)
            t_deq = P._time(lambda: (MX4.mx4_dequant_frag(q, s, deq, N, K), H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi)),
                            args.reps)
            print(json.dumps({"probe": "prefill_chunk", "M": M, "kind": kind, "mxfp4_gemm_us": round(t_mx, 2),
                              "dequant_plus_gemm_pf_us": round(t_deq, 2)}), flush=True)
            del q, s, deq, wsp
            torch.cuda.empty_cache()


def sweep(args):
    """Every explicit decomposition of ssd_gemm_mxfp4_cfg at M = 8 (8 weight copies per launch shape)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import mx4_ops as MX4
    dev = torch.device("cuda", 0)
    M, COPIES = 8, 8
    for model in args.models.split(","):
        for kind, (N, K, epi) in P._shapes(P.MODELS[model]).items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(16 * N, dtype=torch.bfloat16, device=dev)
            ws = [_mx4(N, K, dev) for _ in range(COPIES)]
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            nbytes = mx4_bytes(N, K)
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
                                    MX4.gemm_mxfp4(x, w[0], w[1], y, M, N, K, ldy, epi, cfg=cfg)
                            res.append((P._time(run, args.reps) / COPIES, nt, deep, waves, tpw))

            def run_default():
                for w in ws:
                    MX4.gemm_mxfp4(x, w[0], w[1], y, M, N, K, ldy, epi)
            d_us = P._time(run_default, args.reps) / COPIES
            res.sort()
            for us, nt, deep, waves, tpw in res[:4]:
                print(json.dumps({"probe": "sweep", "model": model, "kind": kind, "N": N, "K": K, "nt": nt, "deep": deep, "waves": waves,
                                  "tpw": tpw, "us": round(us, 2), "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
            print(json.dumps({"probe": "sweep_default", "model": model, "kind": kind, "us": round(d_us, 2),
                              "frac_8TBs": round(nbytes / (d_us * 1e-6) / HBM, 4)}), flush=True)
            del ws
            torch.cuda.empty_cache()


def ktable(args):
    import sqlite3
    db = sqlite3.connect(args.db)
    rows = db.execute("select name, duration from kernels where name like '%wq_gemm_kernel%' order by start").fetchall()
    per = (args.reps + 1) * 8
    shapes = {"qkv": (10240, 8192), "o_proj": (8192, 8192), "gate_up": (57344, 8192), "down_proj": (8192, 28672)}
    print("kind,N,K,dtype,pass,kernel,calls,avg_us,min_us,bytes,frac_8TBs")
    i = 0
    for kind, (N, K) in shapes.items():
        for p, dtype in enumerate(PASSES):
            run = rows[i:i + per]
            i += per
            names = {r[0].split("(")[0] for r in run}
            assert len(run) == per and len(names) == 1, (kind, dtype, names)
            d = [r[1] / 1e3 for r in run]
            avg = sum(d) / len(d)
            nbytes = {"fp8": N * K + 4 * N, "w4a16": P.w4_bytes(N, K), "mxfp4": mx4_bytes(N, K)}[dtype]
            print(f"{kind},{N},{K},{dtype},{p},{names.pop()},{len(d)},{avg:.2f},{min(d):.2f},{nbytes},{nbytes / (avg * 1e-6) / HBM:.4f}")


def qerr(args):
    from ssd_amd import quant, weights as W
    torch.manual_seed(0)
    mats = {"N(0, 0.02) [4096, 4096]": (torch.randn(4096, 4096) * 0.02).to(torch.bfloat16)}
    recipe = {"kind": "pair", "shared": 2048, "snr": 8.0, "layer_gain": 0.005}
    for name, shape in (("model.layers.3.mlp.down_proj.weight", (8192, 28672 // 4)), ("model.layers.3.self_attn.o_proj.weight", (8192, 8192))):
        t = W.synthetic_tensor(name, shape, 0, 0.02, "cpu", 0.0, recipe)
        mats[f"pair {name.split('.')[-2]} {list(shape)}"] = t[:2048].contiguous()
    for what, w in mats.items():
        f = w.float()
        rel = lambda d: round(((d.float() - f).norm() / f.norm()).item(), 5)
        print(json.dumps({"probe": "quant_error", "matrix": what, "mxfp4": rel(quant.dequantize_mxfp4(*quant.quantize_mxfp4(w))),
                          "w4a16": rel(quant.dequantize_w4a16(*quant.quantize_w4a16(w))),
                          "fp8": rel(quant.dequantize_fp8(*quant.quantize_fp8(w)))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gemm", "sweep", "step", "ktable", "qerr"])
    ap.add_argument("--db", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--quant", default="mxfp4", choices=["none", "fp8", "w4a16", "mxfp4"])
    ap.add_argument("--models", default="1b,8b,70b,qwen3-32b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"gemm": gemm, "sweep": sweep, "step": P.step, "ktable": ktable, "qerr": qerr}[a.mode](a)
