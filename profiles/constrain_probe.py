"""Token-constraint kernel (include/ssd_hip_constrain.h) measurements on one MI355X.

  python profiles/constrain_probe.py kernel [--reps 200 --passes 5]
      ssd_constrain_rows at V = 128256 for 1, 8 and 24 rows (one sequence per row): an allow mask of 1000 ids alone, the sparse lists
      alone (8 stop ids held back by min_left, 16 bad words of 1 to 4 tokens against a 15-token tail), and everything together,
      against ssd_row_lse and ssd_penalize_rows (a 512-entry history table) on rows of the same shape, alternating in the same process.
      HIP events around `reps` back-to-back launches; every figure is the median of `passes` such timings.  Rows are N(0, 2^2) logits.
  python profiles/constrain_probe.py step [--tokens 256 --passes 4]
      a synchronous speculation step of the Llama-3.1-8B + Llama-3.2-1B shapes (K = 6, jit_speculate, b = 1, the correlated pair of
      bench.py) at temperature 0.7, without and with allowed_token_ids of 1000 ids, alternating in one engine: host clock around
      generate() (which ends in a device synchronise, uploads included) over the number of speculation steps it took.
Prints one JSON line per measurement; profiles/constrain_commands.txt has the command lines behind profiles/constrain_probe.json."""
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

import numpy as np  # noqa: E402
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
    from ssd_amd.hip import penalty_ops as P
    from ssd_amd.hip import constrain_ops as C
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    for T in (1, 8, 24):
        g = torch.Generator().manual_seed(T)
        rows = {k: (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev) for k in ("mask", "sparse", "all", "lse", "pen")}
        W = C.mask_words(V)
        bits = np.zeros((T, W), np.uint32)
        for b in range(T):
            ids = rng.choice(V, size=1000, replace=False)
            np.bitwise_or.at(bits[b], ids >> 5, np.left_shift(np.uint32(1), (ids & 31).astype(np.uint32)))
        allow = dict(allow_on=i32(np.ones(T)), allow_bits=torch.from_numpy(bits.view(np.int32).copy()).to(dev))
        tail = rng.integers(0, V, size=(T, C.TAIL_LD))
        tok, off = np.zeros((T, C.MAX_WORD_TOKENS), np.int64), np.zeros((T, C.MAX_WORDS + 1), np.int64)
        for b in range(T):
            n = 0
            for w in range(16):
                L = 1 + w % 4
                tok[b, n:n + L - 1] = tail[b, C.TAIL_LD - (L - 1):]          # every word matches: the most work
                tok[b, n + L - 1] = rng.integers(0, V)
                n += L
                off[b, w + 1] = n
        stop = np.zeros((T, C.MAX_STOP), np.int64)
        stop[:, :8] = rng.integers(0, V, size=(T, 8))
        sparse = dict(min_left=i32(np.full(T, 4)), stop_ids=i32(stop), stop_len=i32(np.full(T, 8)), bw_tok=i32(tok), bw_off=i32(off),
                      bw_n=i32(np.full(T, 16)), tail=i32(tail), tail_ld=C.TAIL_LD, tail_len=i32(np.full(T, C.TAIL_LD)))
        temps = torch.full((T,), 0.8, dtype=torch.float32, device=dev)
        lse = torch.zeros(T, dtype=torch.float32, device=dev)
        L = 512
        tab_ids = i32(np.stack([rng.choice(V, size=L, replace=False) for _ in range(T)]))
        tab_cnt = i32(np.full((T, L), P.pack_count(1, True)))
        tab_bias = torch.zeros(T, L, dtype=torch.float32, device=dev)
        tab_len = i32(np.full(T, L))
        par = [torch.full((T,), v, dtype=torch.float32, device=dev) for v in (1.1, 0.1, 0.1)]
        cases = {
            "constrain_mask": lambda: C.constrain_rows(rows["mask"], V, T, V, 1, **allow),
            "constrain_sparse": lambda: C.constrain_rows(rows["sparse"], V, T, V, 1, **sparse),
            "constrain_all": lambda: C.constrain_rows(rows["all"], V, T, V, 1, **allow, **sparse),
            "row_lse": lambda: H.row_lse(rows["lse"], V, T, V, temps, 1, lse),
            "penalize_rows": lambda: P.penalize_rows(rows["pen"], V, T, V, 1, tab_ids, tab_cnt, tab_bias, L, tab_len, *par),
        }
        res = {name: [] for name in cases}
        for _ in range(args.passes):               # alternate: one timing of every kernel per pass
            for name, fn in cases.items():
                res[name].append(_time(fn, args.reps))
        med = {name: statistics.median(v) for name, v in res.items()}
        torch.cuda.synchronize()
        kept = int((rows["mask"].view(torch.int16) != -128).sum().item())          # 0xFF80 as int16
        o = {"probe": "constrain_kernel", "V": V, "rows": T, "reps": args.reps, "passes": args.passes,
             "median_us": {k: round(v, 2) for k, v in med.items()},
             "spread_us (max - min over the passes)": {k: round(max(v) - min(v), 2) for k, v in res.items()},
             "constrain_all_over_row_lse": round(med["constrain_all"] / med["row_lse"], 3),
             "constrain_all_over_penalize_rows": round(med["constrain_all"] / med["penalize_rows"], 3),
             "entries_left_by_the_mask (1000 per row)": kept}
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
    allowed = sorted(random.sample(range(V), 1000))

    def run(con):
        sp = SamplingParams(temperature=0.7, ignore_eos=True, max_new_tokens=args.tokens, allowed_token_ids=allowed if con else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, m = eng.generate([prompt], sp, use_tqdm=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lens = list(m["accepted_suffix_lens_with_recovery"])
        return dt * 1e3 / max(1, len(lens)), sum(lens) / max(1, len(lens)), out[0]["token_ids"]

    for con in (False, True):          # warm-up: weights, graphs of both forms, the prefill shape
        run(con)
        run(con)
    res = {"plain": [], "allowed_1000": []}
    acc = {"plain": [], "allowed_1000": []}
    inside = []
    for p in range(args.passes):
        for name, con in (("plain", False), ("allowed_1000", True)):
            ms, mean_len, toks = run(con)
            res[name].append(ms)
            acc[name].append(mean_len)
            if con:
                inside.append(set(toks) <= set(allowed))
    print(json.dumps({"probe": "constrain_step", "shapes": "llama-3.1-8b + llama-3.2-1b, synchronous, K = 6, b = 1, temperature 0.7",
                      "tokens": args.tokens, "passes": args.passes,
                      "ms_per_step (generate wall time incl. prefill / speculation steps), median": {k: round(statistics.median(v), 4)
                                                                                                      for k, v in res.items()},
                      "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in res.items()},
                      "mean_accepted_len": {k: round(statistics.mean(v), 3) for k, v in acc.items()},
                      "every_token_inside_the_set": inside}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=256)
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "step": step}[a.mode](a)
