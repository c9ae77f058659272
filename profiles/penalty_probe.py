"""Logit penalty (repetition / presence / frequency penalty, logit bias; include/ssd_hip_penalty.h) measurements on one MI355X, HIP events
throughout.

  python profiles/penalty_probe.py kernel [--reps 200]
      ssd_penalize_rows at V = 128256 with a 4096-entry history table per sequence (r = 1.1, p = 0.5, f = 0.25, every 16th entry
      biased) for 1, 8 and 24 rows, each row a sequence of its own, and ssd_row_lse on the same rows as the yardstick, alternating
      twice in the same process.  The kernel works in place, so every timed launch is preceded by a device copy that restores the
      rows; the copy alone is timed too and subtracted.  Rows are seeded N(0, 2^2) logits.
  python profiles/penalty_probe.py step [--steps 40 --warmup 10]
      one synchronous-speculation step (K = 6, JIT) of the 8B + 1B shapes (bench.py's c2 models, synthetic weights) at temperature
      0.7, without and with repetition_penalty = 1.1 (history upload on the draft and the target runner included), alternating
      twice in the same process: ms per step and the accepted length.
  python profiles/penalty_probe.py async [--steps 40 --warmup 10]
      bench.py's default c4 workload (70B + 1B shapes, asynchronous speculation k = 7 f = 3, draft co-located, greedy) without and
      with repetition_penalty = 1.1, alternating twice in the same process: mean accepted length, cache hit rate and ms per step.
      The asynchronous draft is not penalised, so the drop in accepted length is the price of the target adjusting alone.
Prints one JSON line per measurement; profiles/penalty_commands.txt has the command lines behind profiles/penalty_probe.json."""
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
TAB = 4096
PARAMS = dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)


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
    dev = torch.device("cuda", 0)
    for T in (1, 8, 24):
        g = torch.Generator().manual_seed(T)
        src = (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev)
        rows = src.clone()
        lse = torch.zeros(T, dtype=torch.float32, device=dev)
        temps = torch.full((T,), 0.7, device=dev)
        ids = torch.stack([torch.randperm(V, generator=g)[:TAB] for _ in range(T)]).to(torch.int32).to(dev)
        cnt = (torch.randint(0, 4, (T, TAB), generator=g) * 2 + torch.randint(0, 2, (T, TAB), generator=g)).to(torch.int32).to(dev)
        bias = torch.zeros(T, TAB)
        bias[:, ::16] = 2.5
        bias = bias.to(dev)
        lens = torch.full((T,), TAB, dtype=torch.int32, device=dev)
        rep = torch.full((T,), PARAMS["repetition_penalty"], device=dev)
        pres = torch.full((T,), PARAMS["presence_penalty"], device=dev)
        freq = torch.full((T,), PARAMS["frequency_penalty"], device=dev)

        def run():
            rows.copy_(src)
            P.penalize_rows(rows, V, T, V, 1, ids, cnt, bias, TAB, lens, rep, pres, freq)
        res = {"copy": [], "row_lse": [], "penalize": []}
        for _ in range(2):
            res["copy"].append(_time(lambda: rows.copy_(src), args.reps))
            res["row_lse"].append(_time(lambda: H.row_lse(src, V, T, V, temps, 1, lse), args.reps))
            res["penalize"].append(_time(run, args.reps) - res["copy"][-1])
        changed = int((rows != src).sum().item())
        print(json.dumps({"probe": "penalty_kernel", "V": V, "table_entries": TAB, "rows": T, "reps": args.reps, "params": PARAMS,
                          "copy_us": [round(v, 2) for v in res["copy"]], "row_lse_us": [round(v, 2) for v in res["row_lse"]],
                          "penalize_us": [round(v, 2) for v in res["penalize"]],
                          "penalize_over_row_lse": round(sum(res["penalize"]) / sum(res["row_lse"]), 3),
                          "entries_changed_per_row": round(changed / T, 1)}), flush=True)


def _timed_steps(engine, prompt, K, args, name, kw, i, probe, temperature):
    from ssd_amd.engine.llm_engine import METRICS
    from ssd_amd.sampling_params import SamplingParams
    total = args.warmup + args.steps
    dev = torch.device("cuda", 0)
    engine.add_request(prompt, SamplingParams(temperature=temperature, ignore_eos=True, max_new_tokens=total * (K + 1) + 8, **kw))
    for k_ in list(METRICS):
        METRICS[k_] = [] if isinstance(METRICS[k_], list) else 0
    st = engine.create_inference_step(engine.config)
    engine.step(st)
    for _ in range(args.warmup):
        engine.step(st)
    n0 = len(METRICS["accepted_suffix_lens_with_recovery"])
    h0 = len(METRICS.get("cache_hits", []))
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    s.record()
    for _ in range(args.steps):
        engine.step(st)
    e.record()
    torch.cuda.synchronize(dev)
    ms = s.elapsed_time(e) / args.steps
    lens = list(METRICS["accepted_suffix_lens_with_recovery"][n0:])
    hits = list(METRICS.get("cache_hits", [])[h0:])
    rec = {"probe": probe, "K": K, "temperature": temperature, "sampling": name, "pass": i, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(ms, 4), "mean_accepted_len": round(sum(lens) / max(1, len(lens)), 3)}
    if hits:
        rec["cache_hit_rate"] = round(sum(hits) / len(hits), 3)
    print(json.dumps(rec), flush=True)
    engine.abort_all()
    return ms, rec["mean_accepted_len"]


def _alternate(engine, prompt, K, args, probe, temperature):
    runs = {}
    for i, (name, kw) in enumerate((("plain", {}), ("repetition_penalty_1.1", {"repetition_penalty": 1.1})) * 2):
        runs.setdefault(name, []).append(_timed_steps(engine, prompt, K, args, name, kw, i, probe, temperature))
    a = sum(r[0] for r in runs["plain"]) / 2
    b = sum(r[0] for r in runs["repetition_penalty_1.1"]) / 2
    print(json.dumps({"probe": probe + "_ratio", "plain_ms": round(a, 4), "penalty_ms": round(b, 4), "penalty_over_plain": round(b / a, 4),
                      "added_us_per_step": round((b - a) * 1e3, 1),
                      "plain_mean_accepted_len": [r[1] for r in runs["plain"]],
                      "penalty_mean_accepted_len": [r[1] for r in runs["repetition_penalty_1.1"]],
                      "plain_spread": round(abs(runs["plain"][0][0] - runs["plain"][1][0]) / a, 4),
                      "penalty_spread": round(abs(runs["repetition_penalty_1.1"][0][0] - runs["repetition_penalty_1.1"][1][0]) / b, 4)}),
          flush=True)


def step(args):
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine
    tname, tcfg, dname, dcfg = bench.workload_models("c2")
    K, max_len = 6, 4096
    blocks = -(-(max_len + K + 1) // 256) + 2
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    engine = LLMEngine(tname, hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=1, max_num_seqs=1,
                       max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256, num_kvcache_blocks=blocks,
                       num_draft_kvcache_blocks=blocks, weights_recipe=recipe, jit_speculate=True)
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(128)]
    _alternate(engine, prompt, K, args, "sync_step_8b_1b", 0.7)
    engine.exit()


def async_(args):
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine
    tname, tcfg, dname, dcfg = bench.workload_models("c4")
    K, F, max_len = 7, 3, 8192
    blocks = -(-(max_len + K + 1 + K * (K + 1) * F) // 256) + 2
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    engine = LLMEngine(tname, hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=1, max_num_seqs=1,
                       max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256, num_kvcache_blocks=blocks,
                       num_draft_kvcache_blocks=blocks, weights_recipe=recipe, draft_async=True, async_fan_out=F, jit_speculate=True,
                       inprocess_draft=True, num_draft_gpus=1)
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(128)]
    _alternate(engine, prompt, K, args, "async_step_c4", 0)
    engine.exit()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step", "async"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "step": step, "async": async_}[a.mode](a)
