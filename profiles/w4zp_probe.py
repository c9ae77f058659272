"""W4A16 with zero points (AWQ / GPTQ form: unsigned codes, one bf16 scale and one zero-point byte per row and 128 columns)
measurements on one MI355X; the shared pieces come from w4a16_probe.py.

  python profiles/w4zp_probe.py gemm [--reps 40]
      the 70B verify GEMMs at M = 8: symmetric (ssd_gemm_w4a16) and zero-point (ssd_gemm_w4a16_zp) alternating twice in the same
      process (w4a16, w4zp, w4a16, w4zp: the gap between the two w4a16 passes is the spread a ratio is read against), each launch
      shape over 8 distinct weight copies (> the 256 MiB Infinity Cache), HIP-event time per launch and the fraction of 8 TB/s on
      the bytes each actually streams; then the two prefill routes at M = 32 / 64 / 128 (zero-point GEMM vs dequantize +
      ssd_gemm_pf).  Run it under `rocprofv3 --kernel-trace --stats` for the kernel-level table.
  python profiles/w4zp_probe.py sweep [--reps 10] [--models 70b]
      every explicit decomposition (ssd_gemm_w4a16_zp_cfg) of the four matrices at M = 8: the four fastest per matrix and the default.
  python profiles/w4zp_probe.py step [--zero-point] [--steps 20 --warmup 5]
      the c4 workload exactly as w4a16_probe.py builds it with quantization="w4a16", with or without w4_zero_point: TTFT p50 at 128
      and 2048 prompt tokens, ms per step and the accepted length.
  python profiles/w4zp_probe.py ktable --db OUT/w4zp_results.db
      (no GPU) the per-matrix M = 8 kernel times of a `gemm` run traced with `rocprofv3 --kernel-trace --stats -o w4zp`: the GEMM
      dispatches in launch order come in runs of 41 x 8 per (matrix, pass), in the order the probe launches them; prints CSV with
      the zero-point / symmetric ratio per matrix against the goal (1072 / 1056 bytes x 1.03 + the symmetric spread).
  python profiles/w4zp_probe.py qerr
      (no GPU) relative Frobenius error of the symmetric and zero-point int4 quantizers, mxfp4 and fp8 on N(0, 0.02) matrices (also
      with the mean shifted by half a sigma) and on correlated-pair weights.
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
PASSES = ("w4a16", "w4zp", "w4a16", "w4zp")
BYTE_RATIO, PER_BYTE_LINE = 1072 / 1056, 1.03
COPIES, TIME_WARMUPS = 8, 1          # weight copies per launch shape in `gemm`; un-timed calls P._time makes before its timed ones


def _w4z(N, K, dev):
    q, s = P._w4(N, K, dev)
    z = torch.randint(0, 16, (N * K // 128,), dtype=torch.uint8, device=dev)
    return q, s, z


def w4z_bytes(N, K):
    return P.w4_bytes(N, K) + N * K // 128


def gemm(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w4_ops as W4
    from ssd_amd.hip import w4zp_ops as W4Z
    dev = torch.device("cuda", 0)
    shapes = P._shapes(P.MODELS["70b"])
    M = 8
    for kind, (N, K, epi) in shapes.items():
        x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
        y = torch.empty(max(M, 16) * N, dtype=torch.bfloat16, device=dev)
        ldy = 0 if epi == H.EPI_SILU_FRAG else N
        for i, dtype in enumerate(PASSES):
            ws = [_w4z(N, K, dev) for _ in range(COPIES)]
            nbytes = w4z_bytes(N, K) if dtype == "w4zp" else P.w4_bytes(N, K)

            def run():
                for w in ws:
                    if dtype == "w4zp":
                        W4Z.gemm_w4a16_zp(x, w[0], w[1], w[2], y, M, N, K, ldy, epi)
                    else:
                        W4.gemm_w4a16(x, w[0], w[1], y, M, N, K, ldy, epi)
            us = P._time(run, args.reps) / COPIES
            print(json.dumps({"probe": "verify_gemm", "M": M, "kind": kind, "N": N, "K": K, "dtype": dtype, "pass": i, "us": round(us, 2),
                              "bytes": nbytes, "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
            del ws
            torch.cuda.empty_cache()
    for M in (32, 64, 128):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(M * N, dtype=torch.bfloat16, device=dev)
            q, s, z = _w4z(N, K, dev)
            deq = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
            wsp = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=dev)
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            t_sym = P._time(lambda: W4.gemm_w4a16(x, q, s, y, M, N, K, ldy, epi), args.reps)
            t_zp = P._time(lambda: W4Z.gemm_w4a16_zp(x, q, s, z, y, M, N, K, ldy, epi), args.reps)
            t_deq = P._time(lambda: (W4Z.w4zp_dequant_frag(q, s, z, deq, N, K), H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi)),
                            args.reps)
            print(json.dumps({"probe": "prefill_chunk", "M": M, "kind": kind, "w4a16_gemm_us": round(t_sym, 2),
                              "w4zp_gemm_us": round(t_zp, 2), "dequant_plus_gemm_pf_us": round(t_deq, 2)}), flush=True)
            del q, s, z, deq, wsp
            torch.cuda.empty_cache()


def sweep(args):
    """Every explicit decomposition of ssd_gemm_w4a16_zp_cfg at M = 8 (8 weight copies per launch shape)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w4zp_ops as W4Z
    dev = torch.device("cuda", 0)
    M, COPIES = 8, 8
    for model in args.models.split(","):
        for kind, (N, K, epi) in P._shapes(P.MODELS[model]).items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(16 * N, dtype=torch.bfloat16, device=dev)
            ws = [_w4z(N, K, dev) for _ in range(COPIES)]
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            nbytes = w4z_bytes(N, K)
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
                                    W4Z.gemm_w4a16_zp(x, w[0], w[1], w[2], y, M, N, K, ldy, epi, cfg=cfg)
                            res.append((P._time(run, args.reps) / COPIES, nt, deep, waves, tpw))

            def run_default():
                for w in ws:
                    W4Z.gemm_w4a16_zp(x, w[0], w[1], w[2], y, M, N, K, ldy, epi)
            d_us = P._time(run_default, args.reps) / COPIES
            res.sort()
            for us, nt, deep, waves, tpw in res[:4]:
                print(json.dumps({"probe": "sweep", "model": model, "kind": kind, "N": N, "K": K, "nt": nt, "deep": deep, "waves": waves,
                                  "tpw": tpw, "us": round(us, 2), "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
            print(json.dumps({"probe": "sweep_default", "model": model, "kind": kind, "us": round(d_us, 2),
                              "frac_8TBs": round(nbytes / (d_us * 1e-6) / HBM, 4)}), flush=True)
            del ws
            torch.cuda.empty_cache()


def step(args):
    args.quant = "w4a16"
    print(json.dumps({"probe": "mode", "quant": "w4a16", "w4_zero_point": bool(args.zero_point)}), flush=True)
    P.step(args, engine_kw={"w4_zero_point": True} if args.zero_point else None)


def ktable(args):
    import sqlite3
    db = sqlite3.connect(args.db)
    rows = db.execute("select name, duration from kernels where name like '%wq_gemm_kernel%' order by start").fetchall()
    per = (args.reps + TIME_WARMUPS) * COPIES           # dispatches of one (matrix, pass): P._time runs fn once before timing
    shapes = {kind: (N, K) for kind, (N, K, _) in P._shapes(P.MODELS["70b"]).items()}
    m8 = per * len(PASSES) * len(shapes)                # the M = 8 part of `gemm` comes first ...
    chunk = 2 * (args.reps + TIME_WARMUPS) * 3 * len(shapes)   # ... then the prefill_chunk part: 2 direct GEMMs per (M, matrix)
    assert len(rows) == m8 + chunk, f"{len(rows)} w4a16 GEMM dispatches in the trace, expected {m8} + {chunk}: not a `gemm --reps {args.reps}` run"
    rows = rows[:m8]
    print("kind,N,K,dtype,pass,kernel,calls,avg_us,min_us,bytes,frac_8TBs")
    i, summary = 0, []
    for kind, (N, K) in shapes.items():
        avgs = {}
        for p, dtype in enumerate(PASSES):
            run = rows[i:i + per]
            i += per
            names = {r[0].split("(")[0] for r in run}
            assert len(run) == per and len(names) == 1, (kind, dtype, names)
            name = next(iter(names))                    # last template argument = ZP, mangled or demangled
            assert ("Lb1EEv" in name or name.rstrip().endswith("true>")) == (dtype == "w4zp"), (kind, dtype, names)
            d = [r[1] / 1e3 for r in run]
            avg = sum(d) / len(d)
            avgs.setdefault(dtype, []).append(avg)
            nbytes = w4z_bytes(N, K) if dtype == "w4zp" else P.w4_bytes(N, K)
            print(f"{kind},{N},{K},{dtype},{p},{names.pop()},{len(d)},{avg:.2f},{min(d):.2f},{nbytes},{nbytes / (avg * 1e-6) / HBM:.4f}")
        sym, zp = sum(avgs["w4a16"]) / 2, sum(avgs["w4zp"]) / 2
        spread = abs(avgs["w4a16"][0] - avgs["w4a16"][1]) / sym
        summary.append((kind, zp / sym, spread, BYTE_RATIO * PER_BYTE_LINE + spread))
    print("kind,zp_over_symmetric,symmetric_spread,goal,met")
    for kind, ratio, spread, goal in summary:
        print(f"{kind},{ratio:.4f},{spread:.4f},{goal:.4f},{'yes' if ratio <= goal else 'no'}")


def qerr(args):
    from ssd_amd import quant, weights as W
    torch.manual_seed(0)
    base = torch.randn(512, 4096) * 0.02
    mats = {"N(0, 0.02) [512, 4096]": base.to(torch.bfloat16), "N(0.01, 0.02) [512, 4096]": (base + 0.01).to(torch.bfloat16)}
    recipe = {"kind": "pair", "shared": 2048, "snr": 8.0, "layer_gain": 0.005}
    for name, shape in (("model.layers.3.mlp.down_proj.weight", (8192, 28672 // 4)), ("model.layers.3.self_attn.o_proj.weight", (8192, 8192))):
        t = W.synthetic_tensor(name, shape, 0, 0.02, "cpu", 0.0, recipe)
        mats[f"pair {name.split('.')[-2]} {list(shape)}"] = t[:2048].contiguous()
    for what, w in mats.items():
        f = w.float()
        rel = lambda d: round(((d.float() - f).norm() / f.norm()).item(), 5)
        print(json.dumps({"probe": "quant_error", "matrix": what, "w4a16": rel(quant.dequantize_w4a16(*quant.quantize_w4a16(w))),
                          "w4a16_zero_point": rel(quant.dequantize_w4zp(*quant.quantize_w4a16_zp(w))),
                          "mxfp4": rel(quant.dequantize_mxfp4(*quant.quantize_mxfp4(w))),
                          "fp8": rel(quant.dequantize_fp8(*quant.quantize_fp8(w)))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gemm", "sweep", "step", "ktable", "qerr"])
    ap.add_argument("--db", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--zero-point", action="store_true")
    ap.add_argument("--models", default="70b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"gemm": gemm, "sweep": sweep, "step": step, "ktable": ktable, "qerr": qerr}[a.mode](a)
