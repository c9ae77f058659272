"""Long-prefill measurements: one JSON line per case on stdout.

  python profiles/prefill_sweep.py gemm [--ms 256,512,...]      GEMM micro-sweep: 70B / 8B qkv, o, gate_up (+SiLU) and down at M rows,
                                                                random operands, default dispatch and every tile form (nt 1..4)
  python profiles/prefill_sweep.py ttft [c4|c2] [--lengths ...]  p50 TTFT of one prompt, target + co-located 1B draft, in two modes in
                                                                the same process: "new" (one gemm_pf launch per linear) and "loop"
                                                                (the 128-row chunk loop, forced by raising HipDecoder.LM_MIN_TOKENS)
  --modes new,loop  --samples N                                  (ttft) which modes, samples per case (p50 over them, after a warm-up)
"""
import argparse
import dataclasses
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 2.5e15          # MI355X dense bf16 MFMA peak, FLOP/s
MATS = [("70b.qkv", 10240, 8192, False), ("70b.o", 8192, 8192, False), ("70b.gate_up", 57344, 8192, True), ("70b.down", 8192, 28672, False),
        ("8b.qkv", 6144, 4096, False), ("8b.o", 4096, 4096, False), ("8b.gate_up", 28672, 4096, True), ("8b.down", 4096, 14336, False)]


def gemm_sweep(ms):
    from ssd_amd.hip import ops as H
    BF = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, N, K, silu in MATS:
        wf = (torch.rand(N * K, generator=g, device="cuda") * 2 - 1).to(BF)      # uniform [-1, 1): not zero-filled
        for M in ms:
            xf = (torch.rand(H.frag_numel(M, K), generator=g, device="cuda") * 2 - 1).to(BF)
            y = torch.empty(H.frag_numel(M, N // 2) if silu else M * N, dtype=BF, device="cuda")
            ws = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K), 4) // 4, dtype=torch.float32, device="cuda")
            epi = H.EPI_SILU_FRAG if silu else H.EPI_ROWS
            ldy = 0 if silu else N

            def timed(nt, reps=10):
                for _ in range(2):
                    H.gemm_pf(xf, wf, y, M, N, K, ldy, ws, epilogue=epi, nt=nt)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    H.gemm_pf(xf, wf, y, M, N, K, ldy, ws, epilogue=epi, nt=nt)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / reps

            us = timed(0)
            forms = {}
            for f in (1, 2, 3, 4):
                forms[f] = round(timed(f, 5), 1)
            fl = 2.0 * M * N * K
            print(json.dumps({"case": "gemm", "matrix": label, "M": M, "N": N, "K": K, "us": round(us, 1), "tflops": round(fl / us * 1e-6, 1),
                              "frac_2p5PF": round(fl / us * 1e6 / PEAK, 3), "us_by_form": forms}), flush=True)
            del xf, y, ws
        del wf
        torch.cuda.empty_cache()


def clear_prefill_graphs(eng):
    """Drop every captured prefill hipGraph so that the next prompt of the same length is launched (and captured) anew."""
    seen = []
    for obj in (eng.model_runner, getattr(eng, "draft_runner", None), getattr(getattr(eng, "draft_server", None), "runner", None)):
        if obj is None or id(obj) in seen or not hasattr(obj, "graphs"):
            continue
        seen.append(id(obj))
        for k in [k for k in obj.graphs if k[0] == "prefill"]:
            del obj.graphs[k]
        if hasattr(obj, "_prefill_seen"):
            obj._prefill_seen.clear()
    torch.cuda.synchronize()


def ttft_sweep(wl, lengths, modes, samples):
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model import HipDecoder
    from ssd_amd.sampling_params import SamplingParams
    tname, tcfg, dname, dcfg = bench.workload_models(wl)
    is_async = wl in bench.ASYNC_WORKLOADS
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    Lmax = max(lengths)
    blocks = (Lmax + 256) // 256 + 4
    kw = dict(hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=7 if is_async else 6, num_gpus=1,
              max_num_seqs=1, max_model_len=Lmax + 256, max_num_batched_tokens=Lmax + 256, kvcache_block_size=256, num_kvcache_blocks=blocks,
              num_draft_kvcache_blocks=blocks, weights_recipe=recipe)
    if is_async:
        kw.update(draft_async=True, async_fan_out=3, jit_speculate=True, inprocess_draft=True, num_draft_gpus=1)
    eng = LLMEngine(tname, **kw)
    sp = SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=1)
    base = HipDecoder.LM_MIN_TOKENS
    random.seed(0)
    for L in lengths:
        res = {}
        for mode in modes:
            HipDecoder.LM_MIN_TOKENS = base if mode == "new" else 1 << 30
            clear_prefill_graphs(eng)
            ts = []
            for it in range(samples + 1):
                # a fresh prompt every run: the engine's prefix cache would otherwise serve a repeated prompt's KV blocks
                prompt = [random.randint(0, 10000) for _ in range(L)]
                torch.cuda.synchronize()
                first = []
                t0 = time.perf_counter()
                eng.generate([prompt], sp, use_tqdm=False,
                             stream_callback=lambda sid, toks: first.append(time.perf_counter()) if not first else None)
                torch.cuda.synchronize()
                if it:                      # the first run of a shape is the eager warm-up
                    ts.append((first[0] - t0) * 1e3)
            res[mode] = statistics.median(ts)
            print(json.dumps({"case": "ttft", "workload": wl, "target": tname, "draft": dname, "prompt": L, "mode": mode,
                              "p50_ms": round(res[mode], 2), "samples_ms": [round(t, 2) for t in ts], "lm_min_tokens": base}), flush=True)
        if "new" in res and "loop" in res:
            print(json.dumps({"case": "ttft_speedup", "workload": wl, "prompt": L, "loop_over_new": round(res["loop"] / res["new"], 3)}), flush=True)
    HipDecoder.LM_MIN_TOKENS = base
    eng.exit() if hasattr(eng, "exit") else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gemm", "ttft"])
    ap.add_argument("workload", nargs="?", default="c4")
    ap.add_argument("--ms", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--lengths", default="128,512,2048,8192")
    ap.add_argument("--modes", default="new,loop")
    ap.add_argument("--samples", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.init()
    if a.what == "gemm":
        gemm_sweep([int(m) for m in a.ms.split(",")])
    else:
        ttft_sweep(a.workload, [int(x) for x in a.lengths.split(",")], a.modes.split(","), a.samples)


if __name__ == "__main__":
    main()
