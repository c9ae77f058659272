"""Qwen3-MoE measurements on one MI355X (csrc/moe.hip, ssd_amd/model.py).

  python profiles/moe_probe.py block [--launches 200 --passes 5]
      one layer's routed MLP at the qwen3-30b-a3b shapes (h 2048, 128 experts of width 768, top 8): ssd_moe_route + the grouped up
      GEMM + the grouped down GEMM + ssd_moe_combine, captured once as a hipGraph and replayed, at T = 1, 8, 24, 128, 2048 rows.
      Routes: "spread" (the rows touch min(8 T, 128) distinct experts: the worst case of a verify) and "uniform" (every row draws 8
      experts uniformly).  The yardstick, in the same process and alternating with the block: ssd_gemm_wf on ONE dense matrix that
      holds as many weight bytes as the experts touched (N = touched * 2304 rows of K = 2048), T rows (<= 128: the kernel's limit).
      Every launch alternates between two copies of the expert tables (1.2 GB each: beyond the 256 MiB Infinity Cache).
  python profiles/moe_probe.py pair [--steps 30 --warmup 5]
      qwen3-30b-a3b + qwen3-0.6b on synthetic weights through LLM.generate, asynchronous speculation (k = 7, f = 3, in-process draft),
      one sequence, prompts of 128 and 2048 tokens: ms per step, mean accepted length, TTFT.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

H_, I_, E_, K_ = 2048, 768, 128, 8
COPIES = 2


def _graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def _time(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches // COPIES):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / (launches // COPIES * COPIES)          # us per block


def _logits(T, kind, dev, g):
    """bf16 router logits [T][E] whose top 8 are the wanted routes."""
    l = torch.randn(T, E_, generator=g, device=dev)
    if kind == "spread":
        order = torch.randperm(E_, generator=g, device=dev)
        for t in range(T):
            l[t, order[(torch.arange(K_, device=dev) + K_ * t) % E_]] += 20.0
    return l.to(torch.bfloat16)


def block(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import moe_ops as M
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    gu = [(torch.randn(E_ * 2 * I_ * H_ // 8, generator=g, device=dev) * 0.02).to(bf).repeat(8) for _ in range(COPIES)]   # frag-major: any bits do
    dn = [(torch.randn(E_ * H_ * I_ // 8, generator=g, device=dev) * 0.02).to(bf).repeat(8) for _ in range(COPIES)]
    for T in (1, 8, 24, 128, 2048):
        x = torch.randn(T, H_, generator=g, device=dev).to(bf)
        ids = torch.zeros(T * K_, dtype=torch.int32, device=dev)
        w = torch.zeros(T * K_, dtype=torch.float32, device=dev)
        offs = torch.zeros(E_ + 1, dtype=torch.int32, device=dev)
        perm = torch.zeros(T * K_, dtype=torch.int32, device=dev)
        act = torch.zeros(T * K_, I_, dtype=bf, device=dev)
        d = torch.zeros(T * K_, H_, dtype=bf, device=dev)
        h = torch.zeros(T, H_, dtype=bf, device=dev)
        for kind in (("spread", "uniform") if T <= 24 else ("uniform",)):
            logits = _logits(T, kind, dev, g)

            def moe():
                for a, b in zip(gu, dn):
                    M.moe_route(logits, E_, T, E_, K_, True, ids, w, offs, perm)
                    M.moe_gemm(x, a, offs, perm, act, T, K_, E_, 2 * I_, H_, M.EPI_UP)
                    M.moe_gemm(act, b, offs, perm, d, T, K_, E_, H_, I_, M.EPI_DOWN)
                    M.moe_combine(d, w, h, T, K_, H_)
            gm = _graph(moe)
            torch.cuda.synchronize()
            touched = int(torch.unique(ids).numel())
            rec = {"probe": "moe_block", "T": T, "routes": kind, "experts_touched": touched, "weight_bytes_touched": touched * 3 * I_ * H_ * 2}
            gd = None
            if T <= 128:
                N = touched * 3 * I_
                dense = [(torch.randn(N * H_ // 8, generator=g, device=dev) * 0.02).to(bf).repeat(8) for _ in range(COPIES)]
                xf = torch.randn(H.frag_numel(T, H_), generator=g, device=dev).to(bf)
                y = torch.zeros(T, N, dtype=bf, device=dev)

                def base():
                    for wd in dense:
                        H.gemm(xf, wd, y, T, N, H_, N, H.EPI_ROWS)
                gd = _graph(base)
            tm, tb = [], []
            for _ in range(args.passes):
                tm.append(_time(gm, args.launches))
                if gd is not None:
                    tb.append(_time(gd, args.launches))
            m_us = statistics.median(tm)
            rec.update(block_us=round(m_us, 2), block_spread=round((max(tm) - min(tm)) / m_us, 4),
                       block_TBps=round(rec["weight_bytes_touched"] / m_us / 1e6, 3))
            if tb:
                b_us = statistics.median(tb)
                rec.update(dense_gemm_wf_us=round(b_us, 2), ratio=round(m_us / b_us, 4), dense_TBps=round(rec["weight_bytes_touched"] / b_us / 1e6, 3))
                del dense, xf, y
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()


def pair(args):
    import random
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    K, F = 7, 3
    t0 = time.perf_counter()
    eng = LLMEngine("qwen3-30b-a3b", draft="qwen3-0.6b", speculate=True, speculate_k=K, draft_async=True, async_fan_out=F, jit_speculate=True,
                    inprocess_draft=True, num_gpus=1, max_num_seqs=1, max_model_len=4096, max_num_batched_tokens=4096,
                    gpu_memory_utilization=0.3)
    print(json.dumps({"probe": "engine_init", "s": round(time.perf_counter() - t0, 1),
                      "target_weight_bytes": eng.model_runner.model.weight_bytes()}), flush=True)
    random.seed(0)
    for plen in (128, 2048):
        prompt = [random.randint(0, 151935) for _ in range(plen)]
        ttft = []
        for rep in range(3):
            eng.config.max_steps = 1 + args.warmup + args.steps
            sp = SamplingParams(temperature=0, max_new_tokens=(args.steps + args.warmup) * (K + 1), ignore_eos=True)
            _, metrics = eng.generate([prompt], sp, use_tqdm=False)
            ttft.append(metrics["target_step_times"][0])
            times = metrics["target_step_times"][1 + args.warmup:]
            lens = metrics["accepted_suffix_lens_with_recovery"][args.warmup:]
            eng.abort_all()
        print(json.dumps({"probe": "moe_pair", "prompt_tokens": plen, "k": K, "f": F, "steps": len(times),
                          "ms_per_step": round(1e3 * statistics.median(times), 3),
                          "mean_accepted_len": round(sum(lens) / max(1, len(lens)), 3),
                          "ttft_ms_p50": round(1e3 * statistics.median(ttft), 3), "ttft_ms_all": [round(1e3 * t, 3) for t in ttft]}), flush=True)
    eng.exit()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["block", "pair"])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"block": block, "pair": pair}[a.mode](a)
