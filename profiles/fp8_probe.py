"""FP8 (e4m3 weight-only) target measurements on one MI355X.

  python profiles/fp8_probe.py gemm [--reps 40]
      the 70B verify GEMMs at M = 8, bf16 (ssd_gemm_wf) next to fp8 (ssd_gemm_fp8), each launch shape over 8 distinct weight copies
      (> the 256 MiB Infinity Cache, so every launch streams from HBM), HIP-event time per launch and the fraction of 8 TB/s on the
      bytes each actually streams; then the two prefill routes at M = 64 / 128 (fp8 GEMM vs dequantize + ssd_gemm_pf).  Run it
      under `rocprofv3 --kernel-trace --stats` for the kernel-level table.
  python profiles/fp8_probe.py sweep [--reps 20]
      every explicit decomposition (ssd_gemm_fp8_cfg) of the four 70B matrices at M = 8, the six fastest per matrix and the default.
  python profiles/fp8_probe.py step --quant {none,fp8} [--steps 20 --warmup 5]
      the c4 workload (70B target + 1B draft, async SSD k = 7, f = 3, co-located draft, b = 1, temp 0) built exactly as bench.run
      builds it, plus the quantization keyword: TTFT p50 at 128 and 2048 prompt tokens, ms per step and the accepted length.
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


def gemm(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import quant_ops as Q
    dev = torch.device("cuda", 0)
    h, I, qkv = 8192, 28672, 10240
    shapes = {"qkv": (qkv, h, H.EPI_ROWS), "o_proj": (h, h, H.EPI_ROWS), "gate_up": (2 * I, h, H.EPI_SILU_FRAG), "down_proj": (h, I, H.EPI_ROWS)}
    COPIES = 8
    for M in (8,):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(max(M, 16) * N, dtype=torch.bfloat16, device=dev)
            s = torch.rand(N, device=dev) * 1e-3
            for dtype in ("bf16", "fp8"):
                if dtype == "bf16":
                    ws = [torch.randn(N * K, device=dev).to(torch.bfloat16) * 0.02 for _ in range(COPIES)]
                else:
                    ws = [torch.randint(0, 0x7e, (N * K,), dtype=torch.uint8, device=dev) for _ in range(COPIES)]
                ldy = 0 if epi == H.EPI_SILU_FRAG else N

                def run():
                    for w in ws:
                        if dtype == "bf16":
                            H.gemm(x, w, y, M, N, K, ldy, epi)
                        else:
                            Q.gemm_fp8(x, w, s, y, M, N, K, ldy, epi)
                us = _time(run, args.reps) / COPIES
                nbytes = N * K * (2 if dtype == "bf16" else 1) + (4 * N if dtype == "fp8" else 0)
                print(json.dumps({"probe": "verify_gemm", "M": M, "kind": kind, "N": N, "K": K, "dtype": dtype, "us": round(us, 2),
                                  "bytes": nbytes, "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
                del ws
            torch.cuda.empty_cache()
    # prefill routes for one chunk of M <= 128 rows: the fp8 GEMM itself vs dequantize into bf16 + ssd_gemm_pf
    for M in (64, 128):
        for kind, (N, K, epi) in shapes.items():
            x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
            y = torch.empty(M * N, dtype=torch.bfloat16, device=dev)
            s = torch.rand(N, device=dev) * 1e-3
            q = torch.randint(0, 0x7e, (N * K,), dtype=torch.uint8, device=dev)
            deq = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
            wsp = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=dev)
            ldy = 0 if epi == H.EPI_SILU_FRAG else N
            t_fp8 = _time(lambda: Q.gemm_fp8(x, q, s, y, M, N, K, ldy, epi), args.reps)
            t_deq = _time(lambda: (Q.fp8_dequant_frag(q, s, deq, N, K), H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi)), args.reps)
            t_bf16 = _time(lambda: H.gemm_pf(x, deq, y, M, N, K, ldy, wsp, epilogue=epi), args.reps)
            print(json.dumps({"probe": "prefill_chunk", "M": M, "kind": kind, "fp8_gemm_us": round(t_fp8, 2),
                              "dequant_plus_gemm_pf_us": round(t_deq, 2), "bf16_gemm_pf_us": round(t_bf16, 2)}), flush=True)
            del q, deq, wsp
            torch.cuda.empty_cache()


def sweep(args):
    """Every explicit decomposition of ssd_gemm_fp8_cfg for the 70B verify shapes at M = 8 (8 weight copies per launch shape)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import quant_ops as Q
    dev = torch.device("cuda", 0)
    h, I, qkv = 8192, 28672, 10240
    shapes = {"qkv": (qkv, h, H.EPI_ROWS), "o_proj": (h, h, H.EPI_ROWS), "gate_up": (2 * I, h, H.EPI_SILU_FRAG), "down_proj": (h, I, H.EPI_ROWS)}
    M, COPIES = 8, 8
    for kind, (N, K, epi) in shapes.items():
        x = torch.randn(H.frag_numel(M, K), device=dev).to(torch.bfloat16)
        y = torch.empty(16 * N, dtype=torch.bfloat16, device=dev)
        s = torch.rand(N, device=dev) * 1e-3
        ws = [torch.randint(0, 0x7e, (N * K,), dtype=torch.uint8, device=dev) for _ in range(COPIES)]
        ldy = 0 if epi == H.EPI_SILU_FRAG else N
        nbytes = N * K + 4 * N
        res = []
        for nt in ((2, 4) if epi == H.EPI_SILU_FRAG else (1, 2, 4)):
            for deep in (0, 1):
                for waves in (2, 4, 8):
                    for tpw in (1, 2, 4):
                        cfg = (nt | (deep << 8), waves | (tpw << 8))

                        def run():
                            for w in ws:
                                Q.gemm_fp8(x, w, s, y, M, N, K, ldy, epi, cfg=cfg)
                        us = _time(run, args.reps) / COPIES
                        res.append((us, nt, deep, waves, tpw))
        def run_default():
            for w in ws:
                Q.gemm_fp8(x, w, s, y, M, N, K, ldy, epi)
        d_us = _time(run_default, args.reps) / COPIES
        res.sort()
        for us, nt, deep, waves, tpw in res[:6]:
            print(json.dumps({"probe": "sweep", "kind": kind, "nt": nt, "deep": deep, "waves": waves, "tpw": tpw, "us": round(us, 2),
                              "frac_8TBs": round(nbytes / (us * 1e-6) / HBM, 4)}), flush=True)
        print(json.dumps({"probe": "sweep_default", "kind": kind, "us": round(d_us, 2), "frac_8TBs": round(nbytes / (d_us * 1e-6) / HBM, 4)}),
              flush=True)
        del ws
        torch.cuda.empty_cache()


def step(args):
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
    engine = LLMEngine(tname, quantization=quant, **kw)
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
    ap.add_argument("mode", choices=["gemm", "sweep", "step"])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--quant", default="fp8", choices=["none", "fp8"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"gemm": gemm, "sweep": sweep, "step": step}[a.mode](a)
