"""Per-request seed kernels (include/ssd_hip_seed.h) measurements on one MI355X.

  python profiles/seed_probe.py kernel [--reps 200 --passes 5]
      ssd_sample_rows_seeded against ssd_sample_rows on the same rows at V = 128256 for 1, 8, 24 and 88 rows, temperature 0.8:
      the legacy sampler (one 1024-thread workgroup per row), the sliced sampler with every row unseeded (the legacy stream: three
      mix64 per entry) and with every row seeded (one mix64 per entry), alternating in the same process.  HIP events around `reps`
      back-to-back launches; every figure is the median of `passes` such timings.  ssd_rng_advance is not in the timed window (it
      follows both forms).  The unseeded tokens are compared with the legacy sampler's.  Rows are seeded N(0, 2^2) logits.
  python profiles/seed_probe.py step [--tokens 256 --passes 4]
      a synchronous speculation step of the Llama-3.1-8B + Llama-3.2-1B shapes (K = 6, jit_speculate, b = 1, the correlated pair of
      bench.py) at temperature 0.7, without and with a seed, alternating in one engine: host clock around generate() (which ends in
      a device synchronise) over the number of speculation steps it took.
Prints one JSON line per measurement; profiles/seed_commands.txt has the command lines behind profiles/seed_probe.json."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

V = 128256


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps          # us per call


def kernel(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import seed_ops as S
    dev = torch.device("cuda", 0)
    for T in (1, 8, 24, 88):
        g = torch.Generator().manual_seed(T)
        rows = (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev)
        temps = torch.full((T,), 0.8, dtype=torch.float32, device=dev)
        word = torch.tensor([12345], dtype=torch.int64, device=dev)
        pos = torch.arange(T, dtype=torch.int64, device=dev) + 100
        none = torch.full((T,), -1, dtype=torch.int64, device=dev)
        some = torch.arange(T, dtype=torch.int64, device=dev) + 1
        ws = torch.zeros(S.sample_seeded_ws_bytes(T, V) // 8, dtype=torch.int64, device=dev)
        out = {k: torch.zeros(T, dtype=torch.int64, device=dev) for k in ("legacy", "sliced_unseeded", "sliced_seeded")}
        cases = {
            "legacy": lambda: H.sample_rows(rows, V, T, V, temps, 1, word, 1, out["legacy"]),
            "sliced_unseeded": lambda: S.sample_rows_seeded(rows, V, T, V, temps, 1, word, 1, out["sliced_unseeded"], none, 1, pos,
                                                            S.TARGET, ws),
            "sliced_seeded": lambda: S.sample_rows_seeded(rows, V, T, V, temps, 1, word, 1, out["sliced_seeded"], some, 1, pos,
                                                          S.TARGET, ws),
        }
        res = {name: [] for name in cases}
        for _ in range(args.passes):               # alternate: one timing of every variant per pass
            for name, fn in cases.items():
                res[name].append(_time(fn, args.reps))
        med = {name: statistics.median(v) for name, v in res.items()}
        torch.cuda.synchronize()
        o = {"probe": "seed_kernel", "V": V, "rows": T, "reps": args.reps, "passes": args.passes,
             "median_us": {k: round(v, 2) for k, v in med.items()},
             "spread_us (max - min over the passes)": {k: round(max(v) - min(v), 2) for k, v in res.items()},
             "sliced_seeded_over_legacy": round(med["sliced_seeded"] / med["legacy"], 3),
             "sliced_unseeded_over_legacy": round(med["sliced_unseeded"] / med["legacy"], 3),
             "unseeded_tokens_equal_legacy": bool(torch.equal(out["legacy"], out["sliced_unseeded"]))}
        print(json.dumps(o), flush=True)


def step(args):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import PRESETS
    from ssd_amd.sampling_params import SamplingParams
    K, max_len = 6, 2048
    tcfg, dcfg = PRESETS["llama-3.1-8b"], dataclasses.replace(PRESETS["llama-3.2-1b"], tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}     # bench.py's pair
    blocks = -(-(max_len + K + 1) // 256) + 2
    eng = LLMEngine("llama-3.1-8b", hf_config=tcfg, draft="llama-3.2-1b", draft_hf_config=dcfg, speculate=True, speculate_k=K,
                    jit_speculate=True, max_num_seqs=1, max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256,
                    num_kvcache_blocks=blocks, num_draft_kvcache_blocks=blocks, weights_recipe=recipe)
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(128)]

    def run(seed):
        sp = SamplingParams(temperature=0.7, ignore_eos=True, max_new_tokens=args.tokens, seed=seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, m = eng.generate([prompt], sp, use_tqdm=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lens = list(m["accepted_suffix_lens_with_recovery"])
        return dt * 1e3 / max(1, len(lens)), sum(lens) / max(1, len(lens)), out[0]["token_ids"]

    for seed in (None, 1):          # warm-up: weights, graphs of both forms, the prefill shape
        run(seed)
        run(seed)
    res = {"unseeded": [], "seeded": []}
    acc = {"unseeded": [], "seeded": []}
    repeat = []
    for p in range(args.passes):
        for name, seed in (("unseeded", None), ("seeded", 1000 + p)):
            ms, mean_len, toks = run(seed)
            res[name].append(ms)
            acc[name].append(mean_len)
            if seed is not None:
                repeat.append(run(seed)[2] == toks)
    print(json.dumps({"probe": "seed_step", "shapes": "llama-3.1-8b + llama-3.2-1b, synchronous, K = 6, b = 1, temperature 0.7",
                      "tokens": args.tokens, "passes": args.passes,
                      "ms_per_step (generate wall time incl. prefill / speculation steps), median": {k: round(statistics.median(v), 4)
                                                                                                      for k, v in res.items()},
                      "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in res.items()},
                      "mean_accepted_len": {k: round(statistics.mean(v), 3) for k, v in acc.items()},
                      "seeded_rerun_gives_the_same_tokens": repeat}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=256)
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "step": step}[a.mode](a)
