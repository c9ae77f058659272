"""Prompt log-probabilities (include/ssd_hip_prompt_logprob.h) measurements on one MI355X, HIP events throughout.

  python profiles/prompt_logprob_probe.py kernel [--reps 200 --passes 5]
      ssd_logprob_rows_known against ssd_logprob_rows + ssd_logprob_pick on the same rows at V = 128256, n_top in {0, 5, 20} and
      T in {8, 128, 512}, alternating in the same process: every figure is the median of `passes` timings of `reps` launches.
  python profiles/prompt_logprob_probe.py chunk [--reps 200 --passes 5]
      the prompt pass of one chunk -- final norm of the chunk's rows, LM head, ssd_logprob_rows_known -- at 128, 256 and 512 rows for
      the 70B head (h = 8192, V = 128256) and the 8B head (h = 4096): time per prompt row, the quantity the runner's
      prompt_logprob_rows default is chosen by.  The decoder is a one-layer model of the head's sizes (the pass touches no layer).
  python profiles/prompt_logprob_probe.py ttft [--samples 5]
      time to first token of a 2048-token prompt, 70B target + 1B draft (synchronous speculation), without and with
      prompt_logprobs=5, alternating in one process.
  python profiles/prompt_logprob_probe.py rows [--grid]
      how tests/test_engine_prompt_logprob_gpu.py's prompts are chosen: per prompt, at how many PROMPT positions the top-5 list of
      the decoder's prefill logits (sorted on the host; none of the log-probability code runs) is not the oracle's, and the largest
      |HIP logit - oracle logit| over those rows (profiles/logprob_probe.py logit_err measures the generated positions).
Prints one JSON line per measurement; profiles/prompt_logprob_probe.json collects them."""
from __future__ import annotations

import argparse
import json
import os
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


def _alternate(cases, reps, passes):
    res = {name: [] for name in cases}
    for _ in range(passes):                        # one timing of every variant per pass
        for name, fn in cases.items():
            res[name].append(_time(fn, reps))
    return ({k: round(statistics.median(v), 2) for k, v in res.items()}, {k: round(max(v) - min(v), 2) for k, v in res.items()})


def kernel(args):
    from ssd_amd.hip import logprob_ops as L
    from ssd_amd.hip import prompt_logprob_ops as P
    dev = torch.device("cuda", 0)
    for T in (8, 128, 512):
        g = torch.Generator().manual_seed(T)
        rows = (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)      # noqa: E731
        lse, out, tv = f32(T), f32(T), f32(T, L.MAX_N)
        lse2, out2, tv2 = f32(T), f32(T), f32(T, L.MAX_N)
        ti = torch.zeros(T, L.MAX_N, dtype=torch.int32, device=dev)
        ti2, rank = torch.zeros_like(ti), torch.zeros(T, dtype=torch.int32, device=dev)
        ws = f32(L.logprob_rows_ws_bytes(T, V) // 4)
        tokens = torch.randint(0, V, (T,), generator=g).to(dev)
        cases = {}
        for n in (0, 5, 20):
            ntop = torch.full((T,), n, dtype=torch.int32, device=dev)

            def pair(ntop=ntop):
                L.logprob_rows(rows, V, T, V, ntop, 1, lse, tv, ti, ws)
                L.logprob_pick(rows, V, T, V, tokens, lse, ntop, 1, out)

            def known(ntop=ntop):
                P.logprob_rows_known(rows, V, T, V, ntop, tokens, lse2, tv2, ti2, out2, rank, ws)
            cases[f"rows_pick_n{n}"], cases[f"known_n{n}"] = pair, known
        med, spread = _alternate(cases, args.reps, args.passes)
        same = bool(torch.equal(lse.view(torch.int32), lse2.view(torch.int32)) and torch.equal(out.view(torch.int32), out2.view(torch.int32))
                    and torch.equal(ti, ti2) and torch.equal(tv.view(torch.int32), tv2.view(torch.int32)))
        print(json.dumps({"probe": "prompt_logprob_kernel", "V": V, "rows": T, "reps": args.reps, "passes": args.passes, "median_us": med,
                          "spread_us (max - min over the passes)": spread,
                          "known_over_rows_pick": {f"n{n}": round(med[f"known_n{n}"] / med[f"rows_pick_n{n}"], 3) for n in (0, 5, 20)},
                          "bits_equal_at_n20": same}), flush=True)


def chunk(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import prompt_logprob_ops as P
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    from ssd_amd import weights as W
    dev = torch.device("cuda", 0)
    for name, h, heads in (("70B head", 8192, 64), ("8B head", 4096, 32)):
        cfg = ModelConfig("llama", h, 1, heads, 8, 128, 1024, V, 1e-5, 5e5, 8192, False)
        dec = HipDecoder(cfg, max_tokens=2048, max_seqs=2, max_blocks=8, block_size=256, max_model_len=2048, device=dev)
        dec.load_weights(W.synthetic_weights(cfg, 0, 0.02, 0, 1, gen_device="cuda", out_device=str(dev)))
        dec.buf_h[:2048].normal_(generator=None)
        dec.buf_res[:2048].normal_(generator=None)
        dec._last = None
        rows_idx = torch.arange(2048, dtype=torch.int32, device=dev)
        tokens = torch.randint(0, V, (2048,), device=dev)
        cases = {}
        for C in (128, 256, 512):
            frag = torch.zeros(H.frag_numel(C, h), dtype=torch.bfloat16, device=dev)
            logits = torch.zeros(C, V, dtype=torch.bfloat16, device=dev)
            ws = torch.zeros(P.logprob_known_ws_bytes(C, V) // 4, dtype=torch.float32, device=dev)
            ntop = torch.full((C,), 5, dtype=torch.int32, device=dev)
            f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
            lse, out, tv = f32(C), f32(C), f32(C, P.MAX_N)
            ti, rank = torch.zeros(C, P.MAX_N, dtype=torch.int32, device=dev), torch.zeros(C, dtype=torch.int32, device=dev)

            def one(C=C, frag=frag, logits=logits, ws=ws, ntop=ntop, lse=lse, out=out, tv=tv, ti=ti, rank=rank):
                dec.compute_logits_into(rows_idx, C, frag, logits)
                P.logprob_rows_known(logits, V, C, V, ntop, tokens, lse, tv, ti, out, rank, ws)

            def head_only(C=C, frag=frag, logits=logits):
                dec.compute_logits_into(rows_idx, C, frag, logits)
            cases[f"pass_{C}"], cases[f"norm_gemm_{C}"] = one, head_only
        med, spread = _alternate(cases, args.reps, args.passes)
        print(json.dumps({"probe": "prompt_logprob_chunk", "head": name, "h": h, "V": V, "n_top": 5, "reps": args.reps, "passes": args.passes,
                          "median_us_per_chunk": med, "spread_us (max - min over the passes)": spread,
                          "us_per_prompt_row": {str(C): round(med[f"pass_{C}"] / C, 3) for C in (128, 256, 512)},
                          "spread_us_per_prompt_row": {str(C): round(spread[f"pass_{C}"] / C, 3) for C in (128, 256, 512)},
                          "chunk_logits_MB": {str(C): round(C * V * 2 / 1e6, 1) for C in (128, 256, 512)}}), flush=True)
        del dec
        torch.cuda.empty_cache()


def ttft(args):
    import dataclasses
    import random
    import bench
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    tname, tcfg, dname, dcfg = bench.workload_models("c3")
    dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
    recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": 8.0, "layer_gain": 0.005}
    K, max_len = 6, 4096
    blocks = -(-(max_len + K + 1) // 256) + 2
    eng = LLMEngine(tname, hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=1, max_num_seqs=1,
                    max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256, num_kvcache_blocks=blocks,
                    num_draft_kvcache_blocks=blocks, weights_recipe=recipe)
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(2048)]
    res = {"off": [], "prompt_logprobs_5": []}
    for i in range(args.samples + 2):
        for name, n in (("off", None), ("prompt_logprobs_5", 5)):
            prompt[0] = (prompt[0] + 1) % 10000        # a new prompt every time: the plain request takes no prefix hit either
            sp = SamplingParams(temperature=0, max_new_tokens=1, ignore_eos=True, prompt_logprobs=n)
            first = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = eng.generate([list(prompt)], sp, use_tqdm=False,
                                  stream_callback=lambda sid, toks: first.append(time.perf_counter()) if not first else None)
            if i >= 2:      # the plain prefill runs eagerly at first sight and captures at the second: steady state from the third
                res[name].append((first[0] - t0) * 1e3)
            assert (n is None) == ("prompt_logprobs" not in out[0]) and (n is None or len(out[0]["prompt_logprobs"]) == 2048)
    med = {k: round(statistics.median(v), 2) for k, v in res.items()}
    print(json.dumps({"probe": "prompt_logprob_ttft", "pair": "70B + 1B shapes, synchronous speculation k = 6", "prompt_tokens": 2048,
                      "samples": args.samples, "prompt_logprob_rows": eng.model_runner.prompt_logprob_rows, "median_ms": med,
                      "all_ms": {k: [round(x, 2) for x in v] for k, v in res.items()},
                      "difference_ms": round(med["prompt_logprobs_5"] - med["off"], 2),
                      "extra_work": "2047 x 8192 x 128256 LM-head GEMM = 4.3 TFLOP, ~1 GB of chunk logits written and read; the plain "
                                    "prefill replays a hipGraph, the scoring one runs eagerly"}), flush=True)


def rows(args):
    from oracle.model import Ctx, OracleModel
    from ssd_amd import weights as W
    from ssd_amd.hip import ops as H
    from ssd_amd.model import AttnMeta, HipDecoder
    from tests.test_engine_temperature_gpu import KW, cfgs
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda", 0)
    t, _ = cfgs()
    wt = W.synthetic_state_dict(t, 0, KW["weights_std"])
    if args.grid:
        A = (3, 5, 9, 11, 13, 15, 17, 19)       # batches of 8 with the row count of the test's (108: the GEMMs of 33..128 rows)
        abn = [(A[(k + i) % 8], b, n) for k in range(8) for i, b, n in ((0, 1, 9), (1, 5, 9), (2, 3, 9), (0, 2, 13), (1, 6, 13), (2, 4, 13),
                                                                       (0, 4, 21), (1, 7, 21))]
    else:
        from tests.prompt_logprob_ref import ENGINE_LONG_ABN, ENGINE_PROMPTS_ABN
        abn = ENGINE_PROMPTS_ABN + [ENGINE_LONG_ABN]
    prompts = [[(a * j + b) % 128 for j in range(n)] for a, b, n in abn]
    model = OracleModel(t, wt, 16, 16)
    bs, nb = 16, 8
    dec = HipDecoder(t, max_tokens=1024, max_seqs=8, max_blocks=nb, block_size=bs, max_model_len=128, device=dev)
    dec.load_weights(iter(wt.items()))
    dec.alloc_kv(8 * nb)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=dev)       # noqa: E731
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device=dev)       # noqa: E731
    top5 = lambda row: torch.sort(-row.double(), stable=True).indices[:5].tolist()     # noqa: E731
    worst, differs, positions = 0.0, 0, 0
    # the engine prefills its waiting requests together, up to max_num_seqs = 8 of them: the same batches here (a batch's row count
    # decides which GEMM kernels run, and with them the rounding of every row)
    for i0 in range(0, len(prompts), 8):
        batch = prompts[i0:i0 + 8]
        B = len(batch)
        ids = [t_ for p in batch for t_ in p]
        pos = [q for p in batch for q in range(len(p))]
        slots = [(b * nb + q // bs) * bs + q % bs for b, p in enumerate(batch) for q in range(len(p))]
        cu = [0]
        for p in batch:
            cu.append(cu[-1] + len(p))
        T = cu[-1]
        bt = torch.tensor([[b * nb + j for j in range(nb)] for b in range(B)], dtype=torch.int32, device=dev)
        dec.forward(i64(ids), i64(pos), T, AttnMeta(H.MODE_CAUSAL, B, max(len(p) for p in batch), i32(slots), i32([len(p) for p in batch]),
                                                    bt, cu_q=i32(cu)))
        n = dec.compute_logits(T)
        got_all = dec.logits[:n].float().cpu()
        for b, (p, key) in enumerate(zip(batch, abn[i0:i0 + 8])):
            n_p = len(p)
            c = torch.tensor([0, n_p], dtype=torch.int32)
            want = model.compute_logits(model.forward(torch.tensor(p), torch.arange(n_p), Ctx(
                "prefill", slot_mapping=torch.arange(n_p, dtype=torch.int32), cu_q=c, cu_k=c))).float()
            got = got_all[cu[b]:cu[b + 1]]
            err = float((got[:n_p - 1] - want[:n_p - 1]).abs().max())
            d = [q for q in range(n_p - 1) if top5(got[q]) != top5(want[q])]
            worst, differs, positions = max(worst, err), differs + len(d), positions + n_p - 1
            print(json.dumps({"probe": "prompt_rows_grid" if args.grid else "prompt_rows", "prompt (a, b, n): (a * j + b) % 128": list(key),
                              "batch_rows": T, "max_abs_hip_minus_oracle_logit": round(err, 6), "prompt_positions": n_p - 1,
                              "positions_where_the_hip_logits_top5_is_not_the_oracles": d}), flush=True)
    print(json.dumps({"probe": "prompt_rows_total", "prompts": len(prompts), "prompt_positions": positions,
                      "max_abs_hip_minus_oracle_logit": round(worst, 6),
                      "positions_where_the_hip_logits_top5_is_not_the_oracles": differs}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "chunk", "ttft", "rows"])
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--grid", action="store_true", help="rows over a grid of candidate prompts instead of the test's")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 200
    with torch.inference_mode():
        {"kernel": kernel, "chunk": chunk, "ttft": ttft, "rows": rows}[a.mode](a)
