"""Logit filter (top_k / top_p / min_p, include/ssd_hip_filter.h) measurements on one MI355X, HIP events throughout.

  python profiles/filter_probe.py kernel [--reps 200]
      ssd_filter_rows at V = 128256 for 8 and 24 rows with all three filters on (temperature 0.7, top_k 50, top_p 0.9, min_p 0.02), each
      filter alone, and ssd_row_lse on the same rows as the yardstick (two passes over a row with the same launch shape), alternating
      twice in the same process (the gap between the two passes of one kernel is the spread a ratio is read against).  The filter
      works in place, so every timed launch is preceded by a device copy that restores the rows; the copy alone is timed too and
      subtracted.  Rows are seeded N(0, 2^2) logits.
  python profiles/filter_probe.py step [--steps 40 --warmup 10]
      one synchronous-speculation step (K = 6, JIT) of the 8B + 1B shapes (bench.py's c2 models, synthetic weights) at temperature
      0.7, without and with top_p = 0.9, alternating twice in the same process: ms per step and the accepted length.
Prints one JSON line per measurement; profiles/filter_commands.txt has the command lines behind profiles/filter_probe.json."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

V = 128256
ALL = (0.7, 50, 0.9, 0.02)
CASES = {"all_three": ALL, "top_k_only": (0.7, 50, 1.0, 0.0), "top_p_only": (0.7, 0, 0.9, 0.0), "min_p_only": (0.7, 0, 1.0, 0.02)}


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
    from ssd_amd.hip import filter_ops as F
    dev = torch.device("cuda", 0)
    for T in (8, 24):
        g = torch.Generator().manual_seed(T)
        src = (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev)
        rows = src.clone()
        lse = torch.zeros(T, dtype=torch.float32, device=dev)
        kept = torch.zeros(T, dtype=torch.int32, device=dev)
        prm = {name: (torch.full((T,), c[0], device=dev), torch.full((T,), c[1], dtype=torch.int32, device=dev),
                      torch.full((T,), c[2], device=dev), torch.full((T,), c[3], device=dev)) for name, c in CASES.items()}
        temps = prm["all_three"][0]
        res = {}
        for i in range(2):
            res.setdefault("copy", []).append(_time(lambda: rows.copy_(src), args.reps))
            res.setdefault("row_lse", []).append(_time(lambda: H.row_lse(src, V, T, V, temps, 1, lse), args.reps))
            for name, (t, k, p, m) in prm.items():
                def run():
                    rows.copy_(src)
                    F.filter_rows(rows, V, T, V, t, k, p, m, 1, kept)
                res.setdefault(name, []).append(_time(run, args.reps) - res["copy"][-1])
                if i == 0:
                    res[name + "_kept_mean"] = round(kept.float().mean().item(), 1)
        lse_us = sum(res["row_lse"]) / 2
        out = {"probe": "filter_kernel", "V": V, "rows": T, "reps": args.reps, "params (T, top_k, top_p, min_p)": CASES,
               "copy_us": [round(v, 2) for v in res["copy"]], "row_lse_us": [round(v, 2) for v in res["row_lse"]]}
        for name in CASES:
            us = sum(res[name]) / 2
            out[name + "_us"] = [round(v, 2) for v in res[name]]
            out[name + "_over_row_lse"] = round(us / lse_us, 2)
            out[name + "_kept_mean"] = res[name + "_kept_mean"]
        print(json.dumps(out), flush=True)


def step(args):
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine, METRICS
    from ssd_amd.sampling_params import SamplingParams
    tname, tcfg, dname, dcfg = bench.workload_models("c2")
    K, max_len = 6, 4096
    blocks = -(-(max_len + K + 1) // 256) + 2
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    engine = LLMEngine(tname, hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=1, max_num_seqs=1,
                       max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256, num_kvcache_blocks=blocks,
                       num_draft_kvcache_blocks=blocks, weights_recipe=recipe, jit_speculate=True)
    dev = torch.device("cuda", 0)
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(128)]
    total = args.warmup + args.steps
    runs = {}
    for i, (name, kw) in enumerate((("plain", {}), ("top_p_0.9", {"top_p": 0.9}), ("plain", {}), ("top_p_0.9", {"top_p": 0.9}))):
        engine.add_request(prompt, SamplingParams(temperature=0.7, ignore_eos=True, max_new_tokens=total * (K + 1) + 8, **kw))
        for k_ in list(METRICS):
            METRICS[k_] = [] if isinstance(METRICS[k_], list) else 0
        st = engine.create_inference_step(engine.config)
        engine.step(st)
        for _ in range(args.warmup):
            engine.step(st)
        n0 = len(METRICS["accepted_suffix_lens_with_recovery"])
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        s.record()
        for _ in range(args.steps):
            engine.step(st)
        e.record()
        torch.cuda.synchronize(dev)
        ms = s.elapsed_time(e) / args.steps
        lens = list(METRICS["accepted_suffix_lens_with_recovery"][n0:])
        runs.setdefault(name, []).append(ms)
        print(json.dumps({"probe": "sync_step_8b_1b", "K": K, "temperature": 0.7, "sampling": name, "pass": i, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": round(ms, 4), "mean_accepted_len": round(sum(lens) / max(1, len(lens)), 3)}),
              flush=True)
        engine.abort_all()
    a, b = sum(runs["plain"]) / 2, sum(runs["top_p_0.9"]) / 2
    print(json.dumps({"probe": "sync_step_8b_1b_ratio", "plain_ms": round(a, 4), "top_p_ms": round(b, 4), "top_p_over_plain": round(b / a, 4),
                      "added_us_per_step": round((b - a) * 1e3, 1), "filter_launches_per_step": "K draft rows + K+1 verify rows = 2K+1 rows",
                      "plain_spread": round(abs(runs["plain"][0] - runs["plain"][1]) / a, 4),
                      "top_p_spread": round(abs(runs["top_p_0.9"][0] - runs["top_p_0.9"][1]) / b, 4)}), flush=True)
    engine.exit()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "step": step}[a.mode](a)
