"""Log-probability kernels (include/ssd_hip_logprob.h) measurements on one MI355X, HIP events throughout.

  python profiles/logprob_probe.py kernel [--reps 200 --passes 5]
      ssd_logprob_rows + ssd_logprob_pick at V = 128256 for 1, 8 and 24 rows, n_top in {0, 5, 20}, without and with the raw copy, and
      ssd_row_lse on the same rows as the yardstick (one workgroup per row over the same bytes), alternating in the same process:
      every figure is the median of `passes` timings of `reps` back-to-back launches.  Rows are seeded N(0, 2^2) logits.
  python profiles/logprob_probe.py logit_err [--grid]
      the largest |HIP logit - oracle logit| of the tiny test target (tests/test_engine_logprob_gpu.py: its models, its prompts, the
      oracle's greedy streams), over the decoder's prefill rows and its single-token decode rows against the oracle's teacher-forced
      bf16 logits: the figure that test's tolerance is twice of; and at how many generated positions the top-5 list of the decoder's
      logits (sorted on the host) is not the oracle's.  Runs none of the log-probability code.
Prints one JSON line per measurement; profiles/logprob_commands.txt has the command lines behind profiles/logprob_probe.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

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
    from ssd_amd.hip import logprob_ops as L
    dev = torch.device("cuda", 0)
    for T in (1, 8, 24):
        g = torch.Generator().manual_seed(T)
        rows = (torch.randn(T, V, generator=g) * 2.0).to(torch.bfloat16).to(dev)
        raw = torch.zeros_like(rows)
        temps = torch.ones(T, dtype=torch.float32, device=dev)
        lse = torch.zeros(T, dtype=torch.float32, device=dev)
        lse2 = torch.zeros(T, dtype=torch.float32, device=dev)
        out = torch.zeros(T, dtype=torch.float32, device=dev)
        tv = torch.zeros(T, L.MAX_N, dtype=torch.float32, device=dev)
        ti = torch.zeros(T, L.MAX_N, dtype=torch.int32, device=dev)
        ws = torch.zeros(L.logprob_rows_ws_bytes(T, V) // 4, dtype=torch.float32, device=dev)
        tokens = torch.randint(0, V, (T,), generator=g).to(dev)
        cases = {}
        for n in (0, 5, 20):
            ntop = torch.full((T,), n, dtype=torch.int32, device=dev)
            for copy in (False, True):
                def rows_only(ntop=ntop, copy=copy):
                    L.logprob_rows(rows, V, T, V, ntop, 1, lse, tv, ti, ws, raw_copy=raw if copy else None, raw_ld=V if copy else 0)

                def rows_pick(ntop=ntop, copy=copy):
                    L.logprob_rows(rows, V, T, V, ntop, 1, lse, tv, ti, ws, raw_copy=raw if copy else None, raw_ld=V if copy else 0)
                    L.logprob_pick(raw if copy else rows, V, T, V, tokens, lse, ntop, 1, out)
                cases[f"rows_n{n}{'_copy' if copy else ''}"] = rows_only
                cases[f"rows_pick_n{n}{'_copy' if copy else ''}"] = rows_pick
        cases["row_lse"] = lambda: H.row_lse(rows, V, T, V, temps, 1, lse2)
        res = {name: [] for name in cases}
        for _ in range(args.passes):               # alternate: one timing of every variant per pass
            for name, fn in cases.items():
                res[name].append(_time(fn, args.reps))
        med = {name: statistics.median(v) for name, v in res.items()}
        torch.cuda.synchronize()
        o = {"probe": "logprob_kernel", "V": V, "rows": T, "reps": args.reps, "passes": args.passes,
             "median_us": {k: round(v, 2) for k, v in med.items()},
             "spread_us (max - min over the passes)": {k: round(max(v) - min(v), 2) for k, v in res.items()},
             "rows_pick_n5_over_row_lse": round(med["rows_pick_n5"] / med["row_lse"], 3),
             "lse_abs_diff_vs_row_lse": round(float((lse - lse2).abs().max()), 6)}
        print(json.dumps(o), flush=True)


def logit_err(args):
    from oracle.model import Ctx, OracleModel
    from oracle.runner import oracle_runner_factory
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.hip import ops as H
    from ssd_amd.model import AttnMeta, HipDecoder
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_engine_logprob_gpu import N_NEW, PROMPTS
    from tests.test_engine_temperature_gpu import KW, cfgs
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda", 0)
    t, _ = cfgs()
    wt = W.synthetic_state_dict(t, 0, KW["weights_std"])
    if args.grid:           # candidate prompts of the same family, one JSON line each: how a prompt set for that test is chosen
        PROMPTS = [[(a * j + b) % 128 for j in range(n)] for a in (3, 5, 7, 9, 11, 13, 15, 17) for b, n in ((1, 9), (2, 7), (4, 12), (6, 10))]
    eng = LLMEngine("t", hf_config=t, max_num_seqs=8, runner_factory=oracle_runner_factory(wt), **KW)
    out = []
    for i in range(0, len(PROMPTS), 8):
        out += eng.generate(PROMPTS[i:i + 8], SamplingParams(temperature=0, max_new_tokens=N_NEW, ignore_eos=True), use_tqdm=False)[0]
    model = OracleModel(t, wt, 16, 16)
    bs = 16
    dec = HipDecoder(t, max_tokens=128, max_seqs=2, max_blocks=8, block_size=bs, max_model_len=128, device=dev)
    dec.load_weights(iter(wt.items()))
    dec.alloc_kv(16)
    table = list(range(8))
    bt = torch.tensor([table], dtype=torch.int32, device=dev)

    def slots(positions):
        return torch.tensor([table[p // bs] * bs + p % bs for p in positions], dtype=torch.int32, device=dev)

    def i64(x):
        return torch.tensor(list(x), dtype=torch.int64, device=dev)

    def i32(x):
        return torch.tensor(list(x), dtype=torch.int32, device=dev)

    def top5(row):
        return torch.sort(-row.double(), stable=True).indices[:5].tolist()

    worst = {"prefill": 0.0, "decode": 0.0}
    differs = {"prefill": 0, "decode": 0}        # positions whose top-5 list (order included) is not the oracle's
    mag = 0.0
    for p, o in zip(PROMPTS, out):
        ids = p + o["token_ids"]
        T, P = len(ids), len(p)
        cu = torch.tensor([0, T], dtype=torch.int32)
        want = model.compute_logits(model.forward(torch.tensor(ids), torch.arange(T), Ctx(
            "prefill", slot_mapping=torch.arange(T, dtype=torch.int32), cu_q=cu, cu_k=cu))).float()
        mag = max(mag, float(want.abs().max()))
        # the whole sequence as one prefill
        dec.forward(i64(ids), i64(range(T)), T, AttnMeta(H.MODE_CAUSAL, 1, T, slots(range(T)), i32([T]), bt, cu_q=i32([0, T])))
        n = dec.compute_logits(T)
        got = dec.logits[:n].float().cpu()
        worst["prefill"] = max(worst["prefill"], float((got - want).abs().max()))
        differs["prefill"] += sum(top5(got[i]) != top5(want[i]) for i in range(P - 1, T - 1))
        # the prompt as a prefill, then the stream token by token
        dec.forward(i64(p), i64(range(P)), P, AttnMeta(H.MODE_CAUSAL, 1, P, slots(range(P)), i32([P]), bt, cu_q=i32([0, P])))
        for i in range(P, T):
            dec.forward(i64([ids[i]]), i64([i]), 1, AttnMeta(H.MODE_CAUSAL, 1, 1, slots([i]), i32([i + 1]), bt, q_per_seq=1))
            dec.compute_logits(1)
            got = dec.logits[:1].float().cpu()
            worst["decode"] = max(worst["decode"], float((got - want[i:i + 1]).abs().max()))
            if i < T - 1:
                differs["decode"] += top5(got[0]) != top5(want[i])
        if args.grid:
            print(json.dumps({"probe": "logit_err_grid", "prompt": p, "running_max_abs_hip_minus_oracle_logit": dict(worst),
                              "running_positions_where_the_hip_logits_top5_is_not_the_oracles": dict(differs)}), flush=True)
    print(json.dumps({"probe": "logit_err", "models": "tiny test target (hidden 256, 2 layers, V = 128, weights_std 0.25)",
                      "prompts": len(PROMPTS), "new_tokens": N_NEW, "max_abs_oracle_logit": round(mag, 4),
                      "max_abs_hip_minus_oracle_logit": {k: round(v, 6) for k, v in worst.items()},
                      "logit_err": round(max(worst.values()), 6), "bound = 2 * logit_err": round(2 * max(worst.values()), 6),
                      "positions": {"prefill": len(PROMPTS) * N_NEW, "decode": len(PROMPTS) * (N_NEW - 1)},
                      "positions_where_the_hip_logits_top5_is_not_the_oracles": differs}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "logit_err"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--grid", action="store_true", help="logit_err over a grid of candidate prompts instead of the test's")
    a = ap.parse_args()
    with torch.inference_mode():
        {"kernel": kernel, "logit_err": logit_err}[a.mode](a)
