"""W4A16 (int4 weight-only, group 128) target measurements on one MI355X.

  python profiles/w4a16_probe.py gemm [--reps 40]
      the 70B verify GEMMs at M = 8, bf16 (ssd_gemm_wf), fp8 (ssd_gemm_fp8) and w4a16 (ssd_gemm_w4a16), each launch shape over 8
      distinct weight copies (> the 256 MiB Infinity Cache, so every launch streams from HBM), HIP-event time per launch and the
      fraction of 8 TB/s on the bytes each actually streams; then the two prefill routes at M = 32 / 64 / 128 (w4a16 GEMM vs
      dequantize + ssd_gemm_pf), which set HipDecoder.W4_DIRECT_MAX_T.  Run it under `rocprofv3 --kernel-trace --stats` for the
      kernel-level table.
  python profiles/w4a16_probe.py sweep [--reps 10]
      every explicit decomposition (ssd_gemm_w4a16_cfg) of the four matrices of the 1B, 8B, 70B and Qwen3-32B at M = 8: the four
      fastest per matrix and the default.
  python profiles/w4a16_probe.py step --quant {none,fp8,w4a16} [--steps 20 --warmup 5]
      the c4 workload (70B target + 1B draft, async SSD k = 7, f = 3, co-located draft, b = 1, temp 0) built exactly as bench.run
      builds it, plus the quantization keyword: TTFT p50 at 128 and 2048 prompt tokens, ms per step and the accepted length.
  python profiles/w4a16_probe.py ktable --db OUT/w4a16_results.db
      (no GPU) the per-matrix M = 8 kernel times of a `gemm` run traced with `rocprofv3 --kernel-trace --stats -o w4a16`: the GEMM
      dispatches in launch order come in runs of 41 x 8 (one warm-up call and --reps 40 timed calls over 8 weight copies) per
      (matrix, dtype), in the order the probe launches them; prints CSV.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM = 8.0e12
MODELS = {
    "1b": dict(nh=32, nkv=8, hd=64, h=2048, I=8192),
    "8b": dict(nh=32, nkv=8, hd=128, h=4096, I=14336),
    "70b": dict(nh=64, nkv=8, hd=128, h=8192, I=28672),
    "qwen3-32b": dict(nh=64, nkv=8, hd=128, h=5120, I=25600),
}


def _shapes(m):
    from ssd_amd.hip import ops as H
    qkv = (m["nh"] + 2 * m["nkv"]) * m["hd"]
    return {"qkv": (qkv, m["h"], H.EPI_ROWS), "o_proj": (m["h"], m["nh"] * m["hd"], H.EPI_ROWS),
            "gate_up": (2 * m["I"], m["h"], H.EPI_SILU_FRAG), "down_proj": (m["h"], m["I"], H.EPI_ROWS)}


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps          # us per call


def _w4(N, K, dev):
    q = torch.randint(0, 256, (N * K // 2,), dtype=torch.uint8, device=dev)
    s = (torch.rand(N * K // 128, device=dev) * 1e-3).to(torch.bfloat16)
    return q, s


def w4_bytes(N, K):
    return N * K // 2 + 2 * (N * K // 128)


def gemm(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import w4_ops as W4
    dev = torch.device("cuda", 0)
    shapes = _shapes(MODELS["70b"])
    COPIES = 8
    M = 8
    for kind, (N, K, epi) in shapes.items():
        x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
        y = torch.empty(max(M, 16) * N, dtype=torch.bfloat16, device=dev)
        s8 = torch.rand(N, device=dev) * 1e-3
        ldy = 0 if epi == H.EPI_SILU_FRAG else N
        for dtype in ("bf16", "fp8", "w4a16"):
            if dtype == "bf16":
                ws = [torch.randn(N * K, device=dev).to(torch.bfloat16) * 0.02 for _ in range(COPIES)]
                nbytes = 2 * N * K
            elif dtype == "fp8":
                ws = [torch.randint(0, 0x7e, (N * K,), dtype=torch.uint8, device=dev) for _ in range(COPIES)]
                nbytes = N * K + 4 * N
            else:
                ws = [_w4(N, K, dev) for _ in range(COPIES)]
                nbytes = w4_bytes(N, K)

            def run():
                for w in ws:
                    if dtype == "bf16":
                        H.gemm(x, w, y, M, N, K, ldy, epi)
                    elif dtype == "fp8":
                        Q.gemm_fp8(x, w, s8, y, M, N, K, ldy, epi)
                    else:
                        W4.gemm_w4a16(x, w[0], w[1], y, M, N, K, ldy, epi)
            us = _time(run, args.reps) / COPIES
            print(json.dumps({"probe": "verify_gemm", "M": M, "kind": kind, "N": N, "K": K, "dtype": dtype, "us": round(us, 2),
                              "bytes": nbytes, "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
            del ws
        torch.cuda.empty_cache()
    # prefill routes for one chunk of M <= 128 rows: the w4a16 GEMM itself vs dequantize into bf16 + ssd_gemm_pf
    for M in (32, 64, 128):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(M * N, dtype=torch.bfloat16, device=dev)
            q, s = _w4(N, K, dev)
            deq = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
            wsp = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=dev)
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            t_w4 = _time(lambda: W4.gemm_w4a16(x, q, s, y, M, N, K, ldy, epi), args.reps)
            t_deq = _time(lambda: (W4.w4_dequant_frag(q, s, deq, N, K), H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi)), args.reps)
            t_bf16 = _time(lambda: H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi), args.reps)
            print(json.dumps({"probe": "prefill_chunk", "M": M, "kind": kind, "w4a16_gemm_us": round(t_w4, 2),
                              "dequant_plus_gemm_pf_us": round(t_deq, 2), "bf16_gemm_pf_us": round(t_bf16, 2)}), flush=True)
            del q, s, deq, wsp
            torch.cuda.empty_cache()


def sweep(args):
    """Every explicit decomposition of ssd_gemm_w4a16_cfg at M = 8 (8 weight copies per launch shape)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w4_ops as W4
    dev = torch.device("cuda", 0)
    M, COPIES = 8, 8
    for model in args.models.split(","):
        for kind, (N, K, epi) in _shapes(MODELS[model]).items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(16 * N, dtype=torch.bfloat16, device=dev)
            ws = [_w4(N, K, dev) for _ in range(COPIES)]
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            nbytes = w4_bytes(N, K)
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
                                    W4.gemm_w4a16(x, w[0], w[1], y, M, N, K, ldy, epi, cfg=cfg)
                            us = _time(run, args.reps) / COPIES
                            res.append((us, nt, deep, waves, tpw))

            def run_default():
                for w in ws:
                    W4.gemm_w4a16(x, w[0], w[1], y, M, N, K, ldy, epi)
            d_us = _time(run_default, args.reps) / COPIES
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
    rows = db.execute("select name, duration from kernels where name like '%gemm_wf_kernel%' or name like '%wq_gemm_kernel%' "
                      "order by start").fetchall()
    per = (args.reps + 1) * 8
    shapes = {"qkv": (10240, 8192), "o_proj": (8192, 8192), "gate_up": (57344, 8192), "down_proj": (8192, 28672)}
    print("kind,N,K,dtype,kernel,calls,avg_us,min_us,bytes,frac_8TBs")
    i = 0
    for kind, (N, K) in shapes.items():
        for dtype in ("bf16", "fp8", "w4a16"):
            run = rows[i:i + per]
            i += per
            names = {r[0].split("(")[0] for r in run}
            assert len(run) == per and len(names) == 1, (kind, dtype, names)
            d = [r[1] / 1e3 for r in run]
            avg = sum(d) / len(d)
            nbytes = {"bf16": 2 * N * K, "fp8": N * K + 4 * N, "w4a16": w4_bytes(N, K)}[dtype]
            print(f"{kind},{N},{K},{dtype},{names.pop()},{len(d)},{avg:.2f},{min(d):.2f},{nbytes},{nbytes / (avg * 1e-6) / HBM:.4f}")


def step(args, engine_kw=None):
    """engine_kw: further LLMEngine keywords (w4zp_probe.py passes w4_zero_point)."""
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine, METRICS
    from ssd_amd.sampling_params import SamplingParams
    tname, tcfg, dname, dcfg = bench.workload_models("c4")
    K, F, max_len = 7, 3, 8192
    lookahead = K + 1 + K * (K + 1) * F
    blocks = -(-(max_len + lookahead) // 256) + 2
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    kw = dict(hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=1, max_num_seqs=1,
              max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256, num_kvcache_blocks=blocks,
              num_draft_kvcache_blocks=blocks, weights_recipe=recipe, draft_async=True, async_fan_out=F, jit_speculate=True,
              inprocess_draft=True, num_draft_gpus=1)
    quant = None if args.quant == "none" else args.quant
    t0 = time.perf_counter()
    engine = LLMEngine(tname, quantization=quant, **(engine_kw or {}), **kw)
    print(json.dumps({"probe": "engine_init", "quant": args.quant, "s": round(time.perf_counter() - t0, 1),
                      "target_weight_bytes": engine.model_runner.model.weight_bytes()}), flush=True)
    dev = torch.device("cuda", 0)
    for n_in in (128, 2048):
        random.seed(0)
        prompt = [random.randint(0, 10000) for _ in range(n_in)]
        ttfts = []
        for _ in range(args.ttft_samples):
            first = []
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            engine.generate([prompt], SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=1), use_tqdm=False,
                            stream_callback=lambda sid, toks: first.append(time.perf_counter()) if not first else None)
            ttfts.append((first[0] - t0) * 1e3)
        kept = ttfts[2:] if len(ttfts) > 2 else ttfts[-1:]
        print(json.dumps({"probe": "ttft", "quant": args.quant, "input_len": n_in, "ttft_p50_ms": round(statistics.median(kept), 2),
                          "samples_ms": [round(t, 2) for t in ttfts]}), flush=True)
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(128)]
    total = args.warmup + args.steps
    engine.add_request(prompt, SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=total * (K + 1) + 8))
    for k_ in list(METRICS):
        METRICS[k_] = [] if isinstance(METRICS[k_], list) else 0
    st = engine.create_inference_step(engine.config)
    engine.step(st)
    for _ in range(args.warmup):
        engine.step(st)
    n0 = len(METRICS["accepted_suffix_lens_with_recovery"])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        engine.step(st)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    lens = list(METRICS["accepted_suffix_lens_with_recovery"][n0:])
    print(json.dumps({"probe": "c4_step", "quant": args.quant, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(dt * 1e3 / args.steps, 4), "mean_accepted_len": round(sum(lens) / max(1, len(lens)), 3),
                      "tokens_per_s": round(sum(lens) / dt, 2)}), flush=True)
    engine.exit()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gemm", "sweep", "step", "ktable"])
    ap.add_argument("--db", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--quant", default="w4a16", choices=["none", "fp8", "w4a16"])
    ap.add_argument("--models", default="1b,8b,70b,qwen3-32b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"gemm": gemm, "sweep": sweep, "step": step, "ktable": ktable}[a.mode](a)
