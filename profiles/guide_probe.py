"""Guided-decoding kernels (include/ssd_hip_guide.h) measurements on one MI355X.

  python profiles/guide_probe.py kernel [--reps 200 --passes 5]
      ssd_guide_walk (chain form, 7 extras) + ssd_guide_rows at V = 128256 for 1, 8 and 24 rows (one sequence and one automaton slot
      per row), with every row standing at
        trie8     a trie state: 8 edges, no default -- nearly the whole row is rewritten;
        open1000  a default with 1000 exceptions (edges to -1) -- 1000 entries are rewritten;
        big70000  a state of 70000 edges, no default -- the search takes both narrowing rounds;
      (the 7 walked tokens are self-loops of that state, so the walk searches it seven times), the walk and the rows kernel also timed
      apart, against ssd_constrain_rows with an allow mask of 1000 ids and ssd_row_lse on rows of the same shape, alternating in the same
      process.  HIP events around `reps` back-to-back launches; every figure is the median of `passes` such timings.  Rows are N(0, 2^2)
      logits.
  python profiles/guide_probe.py step [--tokens 256 --passes 4]
      a synchronous speculation step of the Llama-3.1-8B + Llama-3.2-1B shapes (K = 6, jit_speculate, b = 1, the correlated pair of
      bench.py) at temperature 0.7, without a guide and with guided_choice_ids of four choices of `tokens` tokens, alternating in one
      engine: host clock around generate() (which ends in a device synchronise, uploads included) over the number of speculation steps
      it took.
Prints one JSON line per measurement; profiles/guide_commands.txt has the command lines behind profiles/guide_probe.json."""
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
EXTRAS = 7


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
    from ssd_amd.hip import constrain_ops as C
    from ssd_amd.hip import guide_ops as G
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    # one state per automaton: state 0 with `m` edges, all self-loops (next 0) or all bans (next -1)
    kinds = {"trie8": (8, 0, -1), "open1000": (1000, -1, 0), "big70000": (70000, 0, -1)}          # edges, their next state, the default
    for T in (1, 8, 24):
        g = torch.Generator().manual_seed(T)
        names = list(kinds) + ["mask", "lse"]
        rows = {k: (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev) for k in names}
        cases, tabs = {}, {}
        for name, (m, nxt, dflt) in kinds.items():
            tok = np.stack([np.sort(rng.choice(V, size=m, replace=False)) for _ in range(T)])
            off = np.tile(np.array([0, m]), (T, 1))
            t = (i32(np.ones(T)), i32(off), i32(np.full((T, 1), dflt)), i32(tok), i32(np.full((T, m), nxt)), 1, m)
            # the walked tokens keep the state: an edge's token where the edges are self-loops, any other token under the default
            if nxt == 0:
                ex = np.stack([rng.choice(tok[b], size=EXTRAS + 1) for b in range(T)])
            else:
                ex = np.stack([[x for x in rng.integers(0, V, size=64) if x not in set(tok[b].tolist())][:EXTRAS + 1] for b in range(T)])
            extra = dict(extra=torch.from_numpy(ex.astype(np.int64)).to(dev), extra_ld=EXTRAS + 1, extra_n=i32([EXTRAS]))
            st = torch.full((T,), -1, dtype=torch.int32, device=dev)
            on, s0 = i32(np.ones(T)), i32(np.zeros(T))
            tabs[name] = (t, st)

            def walk(t=t, st=st, on=on, s0=s0, extra=extra):
                G.guide_walk(st, T, 1, on, s0, *t, **extra)

            def ban(name=name, t=t, st=st):
                G.guide_rows(rows[name], V, T, V, st, 1, *t)

            def both(walk=walk, ban=ban):
                walk()
                ban()
            cases[f"guide_{name}"] = both
            cases[f"guide_{name}_walk_alone"] = walk
            cases[f"guide_{name}_rows_alone"] = ban
        W = C.mask_words(V)
        bits = np.zeros((T, W), np.uint32)
        for b in range(T):
            ids = rng.choice(V, size=1000, replace=False)
            np.bitwise_or.at(bits[b], ids >> 5, np.left_shift(np.uint32(1), (ids & 31).astype(np.uint32)))
        allow = dict(allow_on=i32(np.ones(T)), allow_bits=torch.from_numpy(bits.view(np.int32).copy()).to(dev))
        temps = torch.full((T,), 0.8, dtype=torch.float32, device=dev)
        lse = torch.zeros(T, dtype=torch.float32, device=dev)
        cases["constrain_mask"] = lambda: C.constrain_rows(rows["mask"], V, T, V, 1, **allow)
        cases["row_lse"] = lambda: H.row_lse(rows["lse"], V, T, V, temps, 1, lse)
        res = {name: [] for name in cases}
        for _ in range(args.passes):               # alternate: one timing of every kernel per pass
            for name, fn in cases.items():
                res[name].append(_time(fn, args.reps))
        med = {name: statistics.median(v) for name, v in res.items()}
        torch.cuda.synchronize()
        left = {name: int((rows[name].view(torch.int16) != -128).sum().item()) for name in kinds}          # 0xFF80 as int16
        states = {name: sorted(set(tabs[name][1].tolist())) for name in kinds}
        o = {"probe": "guide_kernel", "V": V, "rows": T, "extras_walked": EXTRAS, "reps": args.reps, "passes": args.passes,
             "median_us": {k: round(v, 2) for k, v in med.items()},
             "spread_us (max - min over the passes)": {k: round(max(v) - min(v), 2) for k, v in res.items()},
             "guide_over_constrain_mask": {name: round(med[f"guide_{name}"] / med["constrain_mask"], 3) for name in kinds},
             "guide_over_row_lse": {name: round(med[f"guide_{name}"] / med["row_lse"], 3) for name in kinds},
             "entries_left (8, V - 1000 and 70000 per row)": left, "states_after_the_walk (0: it stayed)": states}
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
    eos = eng.config.eos = eng.scheduler.eos = 128001          # synthetic weights come without a tokenizer: the engine has no EOS of its own
    prompt = [random.randint(0, 10000) for _ in range(128)]
    pool = [t for t in range(V) if t != eos]
    choices = [[random.choice(pool) for _ in range(args.tokens - 1)] for _ in range(4)]

    def run(guided):
        sp = SamplingParams(temperature=0.7, max_new_tokens=args.tokens, **(dict(guided_choice_ids=choices) if guided else dict(ignore_eos=True)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, m = eng.generate([prompt], sp, use_tqdm=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lens = list(m["accepted_suffix_lens_with_recovery"])
        return dt * 1e3 / max(1, len(lens)), sum(lens) / max(1, len(lens)), out[0]["token_ids"]

    for guided in (False, True):          # warm-up: weights, graphs of both forms, the prefill shape
        run(guided)
        run(guided)
    res = {"plain": [], "choice_automaton": []}
    acc = {"plain": [], "choice_automaton": []}
    inside = []
    for p in range(args.passes):
        for name, guided in (("plain", False), ("choice_automaton", True)):
            ms, mean_len, toks = run(guided)
            res[name].append(ms)
            acc[name].append(mean_len)
            if guided:
                inside.append(any(toks == c + [eos] for c in choices))
    print(json.dumps({"probe": "guide_step", "shapes": "llama-3.1-8b + llama-3.2-1b, synchronous, K = 6, b = 1, temperature 0.7",
                      "tokens": args.tokens, "passes": args.passes, "choices": f"4 of {args.tokens - 1} tokens (+ the EOS)",
                      "ms_per_step (generate wall time incl. prefill / speculation steps), median": {k: round(statistics.median(v), 4)
                                                                                                      for k, v in res.items()},
                      "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in res.items()},
                      "mean_accepted_len": {k: round(statistics.mean(v), 3) for k, v in acc.items()},
                      "every_output_is_a_choice_and_the_eos": inside}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=256)
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "step": step}[a.mode](a)
