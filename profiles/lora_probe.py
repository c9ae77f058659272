"""LoRA adapter measurements on one MI355X (csrc/lora.hip, ssd_amd/lora.py).

  python profiles/lora_probe.py kernel [--launches 200 --passes 5]
      the four layer linears of the 70B target at M = 8 and M = 24: ssd_lora_shrink + ssd_lora_expand (the gate_up pair with the
      SiLU epilogue) against that linear's base GEMM on the rows route, alternating in the same process (base, lora, base, lora, ...:
      `passes` readings of `launches` launches each, HIP-event time, the median per side).  Each side is captured once as a hipGraph
      of its 8 launches (pairs) and the replay is timed, as the engine replays them: eager launches through ctypes are host-bound at
      these sizes (two launches cost ~15 us of host time whatever they do).  Slot ranks as max_lora_rank = 16 and 64
      give them (ssd_amd.lora.slot_rank), four slots in the tables; the rows name one slot, or three slots mixed inside the tile.
      Every launch shape runs over 8 distinct weight copies / table copies (> the 256 MiB Infinity Cache for the weights).
  python profiles/lora_probe.py step [--steps 40 --warmup 5]
      a synchronous speculation step of the Llama-3.1-8B target + Llama-3.2-1B draft (K = 6, greedy, one sequence, 128-token prompt):
      no adapter against a rank-16 adapter on all seven modules, alternating twice in the same process; ms per step and mean
      accepted length (the draft is not adapted, so the two legs accept differently and do not share a denominator).
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import w4a16_probe as P  # noqa: E402

COPIES = 8
SLOTS = 4
LINEAR = {"qkv": "qkv", "o_proj": "o", "gate_up": "gate_up", "down_proj": "down"}


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
    return s.elapsed_time(e) * 1e3 / (launches // COPIES * COPIES)          # us per launch (pair)


def kernel(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import lora_ops as L
    from ssd_amd.lora import slot_rank
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    for kind, (N, K, epi) in P._shapes(P.MODELS["70b"]).items():
        ws = [(torch.randn(N * K // 4, device=dev) * 0.02).to(bf).repeat(4) for _ in range(COPIES)]        # frag-major weights: any bits do
        for M in (8, 24):
            x = torch.randn(H.frag_numel(M, K), device=dev).to(bf)
            y = torch.zeros(M, N, dtype=bf, device=dev)
            act = torch.zeros(H.frag_numel(M, N // 2), dtype=bf, device=dev) if epi == H.EPI_SILU_FRAG else None
            wsp = torch.zeros(L.lora_workspace_bytes(M, K, 192) // 4, dtype=torch.float32, device=dev)
            scale = torch.full((SLOTS,), 2.0, dtype=torch.float32, device=dev)

            def base():
                for w in ws:
                    H.gemm(x, w, y, M, N, K, N, H.EPI_ROWS)
            for max_rank in (16, 64):
                R = slot_rank(LINEAR[kind], max_rank)
                a_tabs = [(torch.randn(SLOTS * R * K, device=dev) / K ** 0.5).to(bf) for _ in range(COPIES)]
                b_tabs = [(torch.randn(SLOTS * N * R, device=dev) * 0.02).to(bf) for _ in range(COPIES)]
                for mix, rows in (("one_slot", [1] * M), ("three_slots_mixed", [m % 3 + 1 for m in range(M)])):
                    rs = torch.tensor(rows, dtype=torch.int32, device=dev)

                    def lora():
                        for a, b in zip(a_tabs, b_tabs):
                            L.lora_shrink(x, a, rs, wsp, M, K, R, SLOTS)
                            L.lora_expand(wsp, b, scale, rs, y, N, M, N, K, R, SLOTS, 0, L.EPI_SILU if act is not None else L.EPI_ADD, act)
                    gb, gl = _graph(base), _graph(lora)
                    gb(), gl()
                    torch.cuda.synchronize()
                    tb, tl = [], []
                    for _ in range(args.passes):
                        tb.append(_time(gb, args.launches))
                        tl.append(_time(gl, args.launches))
                    b_us, l_us = statistics.median(tb), statistics.median(tl)
                    print(json.dumps({"probe": "lora_kernel", "kind": kind, "N": N, "K": K, "M": M, "max_lora_rank": max_rank, "R": R,
                                      "rows": mix, "splits": L.lora_default_splits(K), "base_gemm_us": round(b_us, 2),
                                      "shrink_expand_us": round(l_us, 2), "ratio": round(l_us / b_us, 4),
                                      "base_spread": round((max(tb) - min(tb)) / b_us, 4),
                                      "table_bytes_one_slot": 2 * R * (N + K), "weight_bytes": 2 * N * K}), flush=True)
                del a_tabs, b_tabs
                torch.cuda.empty_cache()
        del ws
        torch.cuda.empty_cache()


def step(args):
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.lora import module_shapes
    from ssd_amd.sampling_params import SamplingParams
    import random
    tname, tcfg, dname, dcfg = bench.workload_models("c2")
    K, max_len = 6, 2048
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)      # as bench.py: a tied draft of the pair recipe repeats its input token
    blocks = -(-(max_len + 2 * K + 2) // 256) + 2
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    t0 = time.perf_counter()
    eng = LLMEngine(tname, hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=1, max_num_seqs=1,
                    max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256, num_kvcache_blocks=blocks,
                    num_draft_kvcache_blocks=blocks, weights_recipe=recipe, enable_lora=True, max_loras=1, max_lora_rank=16)
    g = torch.Generator().manual_seed(0)
    tensors = {}
    for li in range(tcfg.num_layers):
        for m, (out, k) in module_shapes(tcfg).items():
            blk = "self_attn" if m in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
            base = f"base_model.model.model.layers.{li}.{blk}.{m}"
            tensors[base + ".lora_A.weight"] = (torch.randn(16, k, generator=g) / k ** 0.5).to(torch.bfloat16)
            tensors[base + ".lora_B.weight"] = (torch.randn(out, 16, generator=g) * 0.002).to(torch.bfloat16)
    eng.add_lora("x", dict(r=16, lora_alpha=32, target_modules=list(module_shapes(tcfg)), tensors=tensors))
    print(json.dumps({"probe": "engine_init", "s": round(time.perf_counter() - t0, 1), "lora_bytes": eng.model_runner.model.lora_bytes(),
                      "target_weight_bytes": eng.model_runner.model.weight_bytes()}), flush=True)
    random.seed(0)
    prompt = [random.randint(0, tcfg.vocab_size - 1) for _ in range(128)]
    for rep in range(2):
        for name in (None, "x"):
            sp = SamplingParams(temperature=0, max_new_tokens=(args.steps + args.warmup) * (K + 1), ignore_eos=True, lora=name)
            eng.config.max_steps = 1 + args.warmup + args.steps      # the prefill, the warm-up rounds, the timed rounds
            _, metrics = eng.generate([prompt], sp, use_tqdm=False)
            times = metrics["target_step_times"][1 + args.warmup:]
            lens = metrics["accepted_suffix_lens_with_recovery"][args.warmup:]
            eng.abort_all()
            print(json.dumps({"probe": "lora_step", "pass": rep, "adapter": name, "steps": len(times),
                              "ms_per_step": round(1e3 * statistics.median(times), 3), "mean_accepted_len": round(sum(lens) / max(1, len(lens)), 3),
                              "ms_per_token": round(1e3 * sum(times) / max(1, sum(lens)), 3)}), flush=True)
    eng.exit()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "step": step}[a.mode](a)
