#!/usr/bin/env python
"""Headline benchmark: speculative decoding output tokens/s on MI355X, the reference's metric
(bench/bench.py:351-361: output tokens / wall clock; decode-only variant llm_engine.py:215-223).

Contract: ``python bench.py --gpus N --steps K --warmup W`` prints ONE JSON line on rank 0.  One rank per GPU: under
``python -m torch.distributed.run --nproc-per-node N`` the ranks are taken from the environment; started as a plain
process with ``--gpus N > 1`` the script re-executes itself under torch.distributed.run on 127.0.0.1 (the reference's
LLM(num_gpus=N) also spawns its own workers, ssd/engine/llm_engine.py:61-93).  A *step* is one full speculation round
of the real engine for one sequence (b = 1) of synthetic token ids -- exactly the objects ``LLM.generate`` drives.

Workload (``--workload``):
  c4   (default; the configuration BASELINE.json's metric is quoted on) Llama-3.1-70B shapes as target + Llama-3.2-1B
       shapes as draft, ASYNCHRONOUS speculation ("SSD") k = 7, fan-out f = 3, b = 1, temp 0, 128-token prompt, KV block
       256, max_model_len 8192, jit backup on a speculation-cache miss (reference README.md:96-97, bench/bench.py:34-51).
       Placement: ``colocated`` -- the target is tensor-parallel over all N GPUs (139 GB of bf16 weights fit one 288 GB
       MI355X, so N = 1 is the same model) and the draft server shares TP rank 0's GPU on its own HIP stream, pre-computing
       the next round's speculation tree while the verify runs; ``dedicated`` -- the last D GPUs (``--draft-dp D``; default:
       all beyond the largest power-of-two target) are a draft group that talks to TP rank 0 over RCCL p2p and shards the
       speculation tree D ways.  Default ``auto``: co-located for N <= 4, dedicated from N = 5 (N = 5: TP 4 + 1 draft GPU =
       BASELINE.json configs[3], the reference's layout; N = 8: TP 4 + draft x4 data-parallel = configs[4]'s layout).
       Same total work at every N -> "strong".
  c3   the same pair, SYNCHRONOUS speculation k = 6 (BASELINE.json configs[2]); draft replicated on every rank.
  c2   Llama-3.1-8B target + 1B draft, sync k = 6 on one GPU (configs[1]).
  c5t  Qwen3-32B target + Qwen3-0.6B draft, async k = 7 f = 3 (configs[4] without the draft data-parallelism).
  c4e  Llama-3.1-70B target + its EAGLE-3 draft (one layer, h 6144, 32000-token head), async k = 7 f = 3 -- the reference's
       `bench.py --eagle`.  ``--eagle-pair constructed`` (default): the target is a correlated-pair target whose head favours the
       draft vocabulary and the draft is wired to compute the target's token map from the token it is fed
       (ssd_amd/weights.py eagle_pair_recipe; through the engine on the CPU oracle: accepted length 3.4-3.9 of 4);
       ``--eagle-pair peaky``: the same three LM-head rows scaled in both models (what rounds 2-3 measured: hits and partial
       acceptance occur, accepted length ~1.05).
  tiny 2-layer toy shapes (plumbing check).
Weights are synthetic (no checkpoints exist offline).  ``--pair correlated`` (default) builds the two models with the
"correlated pair" recipe of ssd_amd/weights.py: real shapes, every matrix streamed in full, values constructed so that
draft and target agree on most greedy tokens -- acceptance, speculation-cache hits and the all-accepted path are
exercised at rates comparable to a trained pair.  ``--pair random`` uses independent N(0, 0.02) weights (acceptance
~0: value = 1 / step latency).  ms_per_step, bytes per step and the roofline fractions are shape-determined and do not
depend on the pair.

A plain run sets up, samples TTFT (the metric's p50), warms up, times ``--steps`` engine steps and prints the line: ``value``,
``ms_per_step``, ``ttft_p50_ms``, ``mean_accepted_len`` and what follows from them arithmetically.  ``--dump-outputs DIR``
writes what the last timed step handed its caller (the sequence's committed tokens, the suffix that step committed, its
recovery token, and the timed steps' accepted lengths and speculation-cache hits) as float64 ``DIR/<name>.npy``; the same
arguments give the same inputs on every run, so two builds can be compared output for output.

With ``--full`` the line also carries the measurements that take runs of their own: ``ttft_first_sighting_ms``, the
reference-protocol run (``reference_protocol``), the independent-draft floor (``random_pair``), ``roofline`` (dominant
kernel family = the skinny weight-streaming GEMMs, timed with HIP events on the launch stream while rotating through all layers' weights so nothing is cache-resident; per-rank shard
shapes at N > 1; where the draft's single-token forwards run as one resident launch per layer, csrc/chain.hip, that launch is
timed as its own kind ``draft.chain_segment.M1``), ``collective`` (N > 1: which all-reduce carries the tensor-parallel sums and its measured latency)
and ``cpu_baseline`` (the oracle engine -- the reference's own modules restated -- timed on the host cores on a
bounded sample; baseline only).
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import random
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # B/s, MI355X spec (guide: 6.29e12 measured copy ceiling)
ASYNC_WORKLOADS = ("c4", "c5t", "c4e")
EAGLE_WORKLOADS = ("c4e", "tiny-eagle")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c4", choices=["c4", "c3", "c2", "c5t", "c4e", "tiny", "tiny-async", "tiny-eagle"])
    ap.add_argument("--k", type=int, default=None, help="speculation length (default: 7 async, 6 sync)")
    ap.add_argument("--f", type=int, default=3, help="async fan-out")
    ap.add_argument("--placement", default="auto", choices=["auto", "colocated", "dedicated"])
    ap.add_argument("--draft-dp", type=int, default=0, help="dedicated placement: draft ranks (data-parallel tree shards); 0 = all ranks beyond the target's")
    ap.add_argument("--pair", default="correlated", choices=["correlated", "random"])
    ap.add_argument("--pair-snr", type=float, default=8.0)
    ap.add_argument("--eagle-pair", default="constructed", choices=["constructed", "peaky"],
                    help="c4e: how target and EAGLE-3 draft are made to agree (ssd_amd/weights.py eagle_pair_recipe / peaky_rows)")
    ap.add_argument("--input-len", type=int, default=128)
    ap.add_argument("--max-model-len", type=int, default=8192)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-random-pair", action="store_true", help="skip the independent-draft leg (value_random_pair)")
    ap.add_argument("--tune-deep", type=int, default=None, choices=(0, 1),
                    help="A/B measurement only (include/ssd_hip_tune.h ssd_tune_deep): 0 = the plain skinny GEMMs of rounds 1-5 for the "
                         "70B-class matrices, 1 = the library default (the DEEP form)")
    ap.add_argument("--ttft-samples", type=int, default=11,
                    help="TTFT runs; the first two are dropped (eager first sighting of the shape, then hipGraph capture)")
    ap.add_argument("--ref-seqs", type=int, default=2, help="sequences of the reference-protocol run (512 output tokens each); 0 = skip")
    ap.add_argument("--ref-output-len", type=int, default=512)
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline figure: first-sighting TTFT, the reference-protocol run, the "
                         "random-pair leg, the GEMM roofline / collective probes and the CPU baseline (--no-* / --ref-seqs 0 skip single ones)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed for its caller as DIR/<name>.npy (float64)")
    return ap.parse_args(argv)


def base_record(args) -> dict:
    """The keys every line of this benchmark carries -- also a FAILURE record (value null + error / stage), so that whoever parses
    "the one JSON line" learns which stage of which rank ended the run (ssd_amd/utils/watchdog.py)."""
    return {"metric": "output tokens/sec + p50 TTFT, Llama-3-70B SSD k=7 f=3; mean accepted len" if args.workload == "c4"
            else "output tokens/sec (speculative decoding, b=1, temp 0), with p50 TTFT and mean accepted length",
            "value": None, "unit": "tokens/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": None,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": args.workload}}


def self_launch(args) -> int:
    """``python bench.py --gpus N`` outside a distributed launch: become the launcher (one rank per GPU).  The launcher is also the
    last line of defence: it relays the ranks' stdout, and if the launch ends -- or outlives SSD_TOTAL_DEADLINE_S and is killed,
    whole process group -- without a JSON line, it prints the failure record itself."""
    import signal
    import threading
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    deadline = float(os.environ.get("SSD_TOTAL_DEADLINE_S", "3000")) + 60.0
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
    seen = []

    def relay():
        for line in p.stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
            t = line.strip()
            if t.startswith("{") and '"metric"' in t:
                seen.append(t)
    th = threading.Thread(target=relay, daemon=True)
    th.start()
    why = None

    def kill_group(sig):
        try:
            os.killpg(p.pid, sig)
        except Exception:
            pass

    # the ranks live in their own session (so that the launcher can kill ALL of them at the deadline): a SIGINT / SIGTERM sent to the
    # launcher -- Ctrl-C, a harness time-out -- must be passed on, or the ranks would keep the GPUs until their own watchdogs end them
    def passed_on(signum, _frame):
        kill_group(signal.SIGTERM)
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            kill_group(signal.SIGKILL)
        os._exit(128 + signum)
    old = {sg: signal.signal(sg, passed_on) for sg in (signal.SIGINT, signal.SIGTERM)}
    try:
        try:
            rc = p.wait(timeout=deadline)
        except subprocess.TimeoutExpired:
            why = f"launch exceeded {deadline:.0f} s: process group killed by the launcher"
            kill_group(signal.SIGKILL)
            rc = p.wait()
    finally:
        if p.poll() is None:            # any other way out of the wait (an exception in the launcher): leave no rank behind
            kill_group(signal.SIGTERM)
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                kill_group(signal.SIGKILL)
        for sg, h in old.items():
            signal.signal(sg, h)
    th.join(timeout=5)
    if not seen:
        rec = base_record(args)
        rec.update({"error": why or f"the launch ended with exit code {rc} without printing a result line", "failure": "launcher",
                    "stage": "unknown (no rank left a record)", "rank": None})
        print(json.dumps(rec), flush=True)
    return rc if rc != 0 else (0 if seen and '"error"' not in seen[-1] else 1)


def workload_models(name):
    from ssd_amd.model_config import PRESETS, ModelConfig
    if name in ("c3", "c4"):
        return "llama-3.1-70b", PRESETS["llama-3.1-70b"], "llama-3.2-1b", PRESETS["llama-3.2-1b"]
    if name == "c2":
        return "llama-3.1-8b", PRESETS["llama-3.1-8b"], "llama-3.2-1b", PRESETS["llama-3.2-1b"]
    if name == "c5t":
        return "qwen3-32b", PRESETS["qwen3-32b"], "qwen3-0.6b", PRESETS["qwen3-0.6b"]
    if name == "c4e":
        return "llama-3.1-70b", PRESETS["llama-3.1-70b"], "eagle3-llama-3.3-70b", PRESETS["eagle3-llama-3.3-70b"]
    if name == "tiny-eagle":
        t = ModelConfig("llama", 512, 4, 8, 8, 64, 1024, 4096, 1e-5, 5e5, 8192, False)
        d = ModelConfig("eagle3", 256, 1, 4, 4, 64, 512, 4096, 1e-5, 5e5, 8192, False, draft_vocab_size=1024, d_model_target=512)
        return "tiny-target", t, "tiny-eagle-draft", d
    t = ModelConfig("llama", 512, 2, 8, 8, 64, 1024, 4096, 1e-5, 5e5, 8192, False)
    d = ModelConfig("llama", 256, 1, 8, 8, 32 * 2, 512, 4096, 1e-5, 5e5, 8192, False)
    return "tiny-target", t, "tiny-draft", d


def gemm_roofline(legs):
    """Time every skinny-GEMM launch shape of one speculation step with HIP events on the launch stream.
    legs: (runner, M rows, forwards of that shape per step).  For each (matrix kind, M) all L layers' matrices are
    launched back to back (L x tens of MB >> the 256 MiB Infinity Cache), so each launch streams its weights from HBM
    as in the real forward; the L launches are captured in a hipGraph and the replay is timed (the real forward is a
    graph replay too; eager launches through ctypes are host-bound for the small shapes)."""
    import torch
    from ssd_amd.utils.graphs import capture
    tot_bytes = tot_time = 0.0
    tot_launch = 0
    per_kind = {}
    for runner, M, fwd_per_step in legs:
        if runner is None or fwd_per_step <= 0:
            continue
        m = runner.model
        L = m.cfg.num_layers
        kinds = [("qkv", m.qkv_n * m.h * 2, lambda li: m.launch_qkv(li, M, runner.d_pos, runner.d_slots, gemm_only=True)),
                 ("o", m.h * m.qn * 2, lambda li: m.launch_o(li, M)),
                 ("gate_up", 2 * m.I * m.h * 2, lambda li: m.launch_gate_up(li, M, gemm_only=True)),
                 ("down", m.h * m.I * 2, lambda li: m.launch_down(li, M))]
        chain = bool(getattr(m, "chain_seg", False)) and M == 1
        if chain:
            # the single-token chain runs the layer's o_proj / gate_up / down_proj and the next layer's QKV as ONE resident launch
            # (csrc/chain.hip): that launch is the kind that is timed, with its own algorithmic bytes
            from ssd_amd.hip import ops as H_

            def seg(li, m=m, runner=runner):
                w, last = m.w, li + 1 == m.cfg.num_layers
                p_ = f"model.layers.{li}."
                nxt = {} if last else dict(
                    w_qkv_next=w[f"model.layers.{li + 1}.self_attn.qkv_proj.weight"], ln_next=w[f"model.layers.{li + 1}.input_layernorm.weight"],
                    positions=runner.d_pos, cos_sin=m.cos_sin, slots=runner.d_slots, q_out=m.buf_q, k_cache=m.kv_cache[li + 1, 0],
                    v_cache=m.kv_cache[li + 1, 1])
                rin, rout = (m.buf_res2, m.buf_res3) if li % 2 == 0 else (m.buf_res3, m.buf_res2)      # (as HipDecoder._forward_chain)
                H_.chain_segment(m.buf_af, rin, m.buf_res if last else rout, w[p_ + "self_attn.o_proj.weight"],
                                 w[p_ + "mlp.gate_up_proj.weight"], w[p_ + "mlp.down_proj.weight"], w[p_ + "post_attention_layernorm.weight"],
                                 m.cfg.rms_norm_eps, m.h, m.qn, m.I, m.qkv_n, m.nh, m.nkv, m.hd, m.block_size, li, m.chain_gr, m.chain_gen,
                                 m.chain_err, h_out=m.buf_h if last else None, **nxt)
            kinds = [("chain_segment", (m.h * m.qn + 3 * m.I * m.h) * 2 + m.qkv_n * m.h * 2 * (L - 1) // L, seg)]
        runner.d_slots[:max(M, 1)].fill_(-1)          # timing only: do not touch the KV cache
        for kind, b, launch in kinds:
            if chain:
                H_.chain_tick(m.chain_gen)
            for li in range(min(2, L)):
                launch(li)
            reps = max(2, 128 // L)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with capture(graph):
                if chain:
                    H_.chain_tick(m.chain_gen)       # (a forward's segments carry its generation in their hand-off tags)
                for li in range(L):
                    launch(li)
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            dt = e0.elapsed_time(e1) * 1e-3 / (reps * L)
            tag = ("draft." if runner.is_draft else "target.") + f"{kind}.M{M}"
            per_kind[tag] = {"us": round(dt * 1e6, 2), "GBps": round(b / dt / 1e9, 1), "MB": round(b / 1e6, 1),
                             "launches_per_step": round(L * fwd_per_step, 1)}
            tot_bytes += b * L * fwd_per_step
            tot_time += dt * L * fwd_per_step
            tot_launch += L * fwd_per_step
    fam = tot_bytes / tot_time
    # The DOMINANT kernel = the launch kind with the largest share of the step's GPU time (the target's gate_up + SiLU GEMM at
    # M = k + 1: gemm_wf_kernel<1,4,1,DEEP> for the 70B): `achieved` / `frac` are ITS algorithmic bytes (2*N*K)
    # over ITS average launch duration, measured live above with HIP events.  The launch-weighted mean over the whole skinny-GEMM
    # family (target + draft, every shape of the step) is reported beside it as `family`.
    dom_tag = max(per_kind, key=lambda t: per_kind[t]["us"] * per_kind[t]["launches_per_step"])
    dom = per_kind[dom_tag]
    dom_bytes = dom["MB"] * 1e6
    achieved = dom_bytes / (dom["us"] * 1e-6)
    out = {"bound": "hbm", "kernel": (f"{dom_tag} (chain_segment_kernel, csrc/chain.hip: o_proj + gate_up + down_proj + next QKV of a single-token "
                                      f"forward in one resident launch)" if "chain_segment" in dom_tag else
                                      f"{dom_tag} (skinny weight-streaming GEMM: gemm_wf_kernel / gemm_fused_kernel, csrc/gemm*.hip)"),
           "achieved": round(achieved / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": round(achieved / HBM_PEAK, 4),
           "traffic": None, "bytes_per_launch": int(dom_bytes), "avg_launch_us": dom["us"],
           "share_of_gemm_time": round(dom["us"] * dom["launches_per_step"] / (tot_time * 1e6), 4),
           "family": {"kernels": "every skinny-GEMM launch of one step (target + draft): gemm_wf_kernel, gemm_sk/sp_kernel, gemm_fused_kernel",
                      "achieved": round(fam / 1e9, 1), "frac": round(fam / HBM_PEAK, 4), "launches_per_step": round(tot_launch, 1),
                      "avg_launch_us": round(tot_time / tot_launch * 1e6, 2), "bytes_per_launch_avg": int(tot_bytes / tot_launch)},
           "per_kind": per_kind}
    # the committed rocprofv3 --kernel-trace --stats summary of the same command (profiles/): its average for this kernel must agree
    if dom_tag.startswith("target.gate_up") and any(r.cfg.hidden_size == 8192 and r.model.tp_size == 1 for r, _, _ in legs if r is not None):
        import glob
        import re
        for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_c4_kernel_stats.txt")), reverse=True):
            try:
                with open(fn) as f:
                    # (round 6: the kernel has a fourth template argument -- DEEP -- and the 70B gate_up runs the `true` form)
                    hit = next((l for l in f if "gemm_wf_kernel<1, 4, 1" in l), None)
                m_ = re.search(r"avg=\s*([0-9.]+)us", hit or "")
                if m_:
                    us = float(m_.group(1))
                    kn = re.search(r"gemm_wf_kernel<[^>]*>", hit)
                    out["rocprof"] = {"from_committed_profile": True, "source": os.path.relpath(fn, ROOT), "kernel": kn.group(0) if kn else "gemm_wf_kernel<1, 4, 1>",
                                      "avg_us": us, "frac": round(dom_bytes / (us * 1e-6) / HBM_PEAK, 4)}
                    break
            except Exception:
                continue
    # HBM traffic per launch: PMC counters cannot be collected from inside this process; the committed separate
    # `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes (profiles/collect.sh; FETCH_SIZE doubled as the gfx950
    # guide prescribes) give read+write bytes = ratio x algorithmic bytes for this kernel family
    # (sub-fields read back from committed files -- NOT observed in this run -- say so: "from_committed_profile")
    for fn in ("traffic_r06.json", "traffic_r05.json", "traffic_r04.json", "traffic_r03.json", "traffic_r02.json", "traffic_r01.json"):
        try:
            with open(os.path.join(ROOT, "profiles", fn)) as f:
                t = json.load(f)
            # the DOMINANT kernel's own counter ratio where the file has it (VERDICT r5 nit: the family ratio 1.0105 was applied
            # to a kernel whose own is 1.0023); the family ratio is reported beside it
            own = next((v.get("ratio") for k, v in t.get("per_kernel", {}).items() if "target" in k and "gate_up" in k), None)
            dom_is_70b_gate_up = any(r.cfg.hidden_size == 8192 for r, _, _ in legs if r is not None)
            ratio = own if (own is not None and dom_is_70b_gate_up) else t["gemm_traffic_over_algorithmic"]
            out["traffic"] = int(dom_bytes * ratio)
            out["traffic_ratio"] = {"dominant_kernel": ratio, "gemm_family": t["gemm_traffic_over_algorithmic"]}
            out["traffic_source"] = {"from_committed_profile": True, "file": "profiles/" + fn, "passes": t.get("source", fn)}
            if "mfma_util" in t and "per_kernel" in t["mfma_util"] and any(r.cfg.hidden_size == 8192 for r, _, _ in legs if r is not None):
                # north_star: "rocprof HBM GB/s and MFMA utilisation against gfx950 peak" -- the separate counter pass of
                # profiles/collect_r02.sh (MfmaUtil / VALUBusy per kernel); the dominant kernel = the 70B gate_up GEMM
                pk = t["mfma_util"]["per_kernel"]
                dom = next((v for k, v in pk.items() if "gate_up" in k and "target" in k), None)
                out["mfma_util"] = {"from_committed_profile": True, "dominant_kernel_pct": None if dom is None else dom.get("MfmaUtil"),
                                    "valu_busy_pct": None if dom is None else dom.get("VALUBusy"),
                                    "range_pct_over_gemm_family": [min(v.get("MfmaUtil", 0) for v in pk.values()),
                                                                   max(v.get("MfmaUtil", 0) for v in pk.values())],
                                    "note": "HBM-bound weight streaming at M <= 8 of 16 MFMA columns: low by construction"}
            break
        except Exception:
            continue
    return out


def collective_probe(engine, M):
    """N > 1: which implementation carries the [M, hidden] bf16 tensor-parallel sums and what one costs (64 of them in
    one hipGraph, every rank in lock step)."""
    import torch
    import torch.distributed as dist
    from ssd_amd.utils.graphs import capture
    m = engine.model_runner.model
    if not m.use_coll:
        return None
    t = torch.zeros(M, m.h, dtype=torch.bfloat16, device=m.device)
    n = 64

    def body():
        for _ in range(n):
            m._allreduce(t)
    body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(g):
        body()
    g.replay()
    torch.cuda.synchronize()
    dist.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (5 * n)
    one_shot = m.custom_ar is not None
    return {"all_reduce": "one-shot full-mesh over hipIpc (csrc/comm.hip)" if one_shot else "RCCL (torch.distributed nccl)",
            "one_shot_validated": one_shot, "one_shot_status": getattr(engine.model_runner, "custom_ar_status", None),
            "fused_add_rmsnorm": bool(one_shot and m.fuse_ar_norm),
            "message_bytes": M * m.h * 2, "avg_us": round(us, 2), "backend": dist.get_backend(m.tp_group)}


def cpu_baseline_reference(cores: int, budget: float):
    """The REFERENCE's own engine classes on the host cores (tests/golden/make_golden.py time_reference_ar: its Scheduler,
    AutoRegressiveStep, ModelRunner.run, LlamaForCausalLM at Llama-3.2-1B shapes, greedy AR, b = 1).  Only possible where
    /root/reference exists (the build container); the GPU box falls back to the port below."""
    import contextlib
    import io
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    with contextlib.redirect_stdout(io.StringIO()):          # the reference prints every step
        import make_golden as MG
        r = MG.time_reference_ar(seconds=budget, threads=cores)
    return {"value": round(r["tokens_per_s"], 3), "unit": "tokens/s", "cores": cores, "kind": "reference",
            "sample": f"the reference's own engine classes (ssd.engine Scheduler / AutoRegressiveStep / ModelRunner.run, LlamaForCausalLM; "
                      f"CUDA-only attention wheels replaced by the fp32 restatement), Llama-3.2-1B shapes (BASELINE configs[0]), greedy AR "
                      f"b=1, 32-token prompt, {r['tokens']} output tokens after 3 untimed steps (torch.compile warm-up), ~{budget:.0f} s sample; "
                      f"prefill {r['prefill_s']:.1f}s incl. compile"}


def cpu_baseline():
    """The CPU path on a bounded sample of the workload: Llama-3.2-1B shapes (the workload's draft model; BASELINE.json
    configs[0]), greedy AR decode, b=1 -> tokens/s.  kind "reference": the reference's own engine classes, when /root/reference
    is importable; kind "port": the oracle engine (reference modules restated on CPU) otherwise (the GPU box).  The 70B target
    does not fit host RAM, so no extrapolation is made -- a baseline, not a target."""
    import torch
    # GEMV-shaped bf16 matmuls stop scaling (and then collapse) beyond a few tens of threads: on the 256-core
    # GPU-box host, 256 threads ran ~1000x slower than 16.  Use at most 16 and report that number as `cores`.
    cores = min(16, os.cpu_count() or 1)
    budget = float(os.environ.get("SSD_BENCH_CPU_SECONDS", "12"))
    if os.path.isdir("/root/reference/ssd") and os.environ.get("SSD_BENCH_CPU_KIND", "") != "port":
        try:
            return cpu_baseline_reference(cores, budget)
        except Exception as e:          # fall through to the port; say why
            print(f"[bench] reference CPU baseline unavailable ({e!r}); timing the port", file=sys.stderr)
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import PRESETS
    from ssd_amd.sampling_params import SamplingParams
    torch.set_num_threads(cores)
    cfg = PRESETS["llama-3.2-1b"]
    from ssd_amd.utils.topology import Topology
    eng = LLMEngine("llama-3.2-1b", hf_config=cfg, runner_factory=oracle_runner_factory(), max_model_len=1024,
                    max_num_batched_tokens=1024, kvcache_block_size=256, num_kvcache_blocks=4,
                    topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1))     # a plain single-process engine at every N
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(32)]
    # time-bounded sample: decode steps until ~12 s of CPU work have been spent (at least 4, at most 512 tokens)
    eng.add_request(prompt, SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=512))
    step = eng.create_inference_step(eng.config)
    t0 = time.perf_counter()
    eng.step(step)                                  # prefill
    t1 = time.perf_counter()
    n = 0
    while not eng.is_finished() and (n < 4 or time.perf_counter() - t1 < budget):
        eng.step(step)
        n += 1
    wall = time.perf_counter() - t0
    dec = n / (time.perf_counter() - t1)
    return {"value": round(dec, 3), "unit": "tokens/s", "cores": cores, "kind": "port",
            "sample": f"oracle engine (CPU restatement of the reference; /root/reference is not present on this box), Llama-3.2-1B shapes "
                      f"(the workload's draft model; BASELINE configs[0]), greedy AR b=1, 32-token prompt, {n} output tokens (time-bounded "
                      f"sample, ~{budget:.0f} s), bf16 weights; end-to-end wall {wall:.1f}s incl. prefill; decode-only rate reported"}


def dump_outputs(out_dir: str, seq, lens, hits) -> None:
    """--dump-outputs: what the last timed step handed its caller, as float64 .npy files (token ids are exact in float64):
    the timed sequence's committed completion tokens, the suffix the last step committed ([recovery, accepted draft tokens...]),
    the recovery token it computed for the next round, and the timed steps' accepted lengths and speculation-cache hits (the
    METRICS that generate() returns).  A few kB at every workload."""
    import numpy as np
    assert seq is not None and lens, "--dump-outputs: the timed request finished before the last timed step"
    comp = list(seq.completion_token_ids)
    arrays = {"completion_token_ids": comp, "last_step_suffix": comp[len(comp) - lens[-1]:],
              "last_step_recovery_token": [seq.recovery_token_id], "accepted_lens": lens, "cache_hits": [float(h) for h in hits]}
    os.makedirs(out_dir, exist_ok=True)
    for name, values in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.asarray(values, dtype=np.float64))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # Whatever fails from here on -- an exception on any rank, a rank that dies and leaves the others waiting in a collective,
    # a hang in code that runs for the first time on a multi-GPU box -- the run ends within a bounded time and rank 0 prints a
    # one-line JSON failure record naming the stage (ssd_amd/utils/watchdog.py).  At N = 1 only the exception path matters.
    from ssd_amd.utils.watchdog import RunGuard
    guard = RunGuard(rank, world, base_record(args)).install()
    guard.run(lambda: run(args, guard, rank, world))


def run(args, guard, rank, world):
    import torch
    import torch.distributed as dist
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    from ssd_amd.engine.llm_engine import LLMEngine, METRICS
    from ssd_amd.sampling_params import SamplingParams

    if args.tune_deep is not None:
        from ssd_amd.hip.lib import load_library
        assert load_library().ssd_tune_deep(args.tune_deep) == 0
    eagle = args.workload in EAGLE_WORKLOADS
    tname, tcfg, dname, dcfg = workload_models("tiny" if args.workload in ("tiny", "tiny-async") else args.workload)
    is_async = args.workload in ASYNC_WORKLOADS or args.workload in ("tiny-async", "tiny-eagle")
    K = args.k if args.k is not None else (7 if is_async else 6)
    max_len = args.max_model_len
    lookahead = (K + 1 + K * (K + 1) * args.f) if is_async else K + 1
    blocks = -(-(max_len + lookahead) // 256) + 2
    recipe = None
    if args.pair == "correlated" and not eagle:
        # a tied draft would predict "repeat the token" (E.E^T is diagonal-dominant): the pair recipe unties the head; the
        # LM-head GEMM streams a [V, h] matrix either way, so bytes and kernels are unchanged
        dcfg = dataclasses.replace(dcfg, tie_word_embeddings=False)
        recipe = {"kind": "pair", "shared": min(dcfg.hidden_size, tcfg.hidden_size), "snr": args.pair_snr, "layer_gain": 0.005}
    if args.pair == "correlated" and eagle and args.eagle_pair == "constructed":
        # the target is a correlated-pair target over nkv * hd shared dims whose head favours the draft vocabulary; the one-layer
        # draft is wired to compute the target's own token map from the token it is fed (one-hot self attention, value = token
        # half - conditioning half): ssd_amd/weights.py _eagle_pair_tensor.  Every matrix keeps its shape and is streamed in full.
        from ssd_amd import weights as W
        recipe = W.eagle_pair_recipe(tcfg, dataclasses.replace(dcfg, d_model_target=tcfg.hidden_size), draft_seed=1,
                                     snr=args.pair_snr)
    elif args.pair == "correlated" and eagle:
        # "peaky" (rounds 2-3): the LM-head rows of the same three tokens scaled in both models (ssd_amd/weights.py peaky_rows):
        # they agree now and then, enough for cache hits, partial acceptance and the extend rows of the glue to run
        recipe = {"kind": "peaky", "gain": 6.0, "peaks": 3, "draft_seed": 1, "draft_vocab": dcfg.draft_vocab_size,
                  "target_vocab": tcfg.vocab_size}
    # placement of the async draft.  auto: up to 4 GPUs every GPU is worth more as a tensor-parallel target rank (the draft
    # server shares rank 0's GPU); from 5 GPUs on the reference's layout pays -- a 4-way tensor-parallel target + the remaining
    # GPUs as a draft group (N = 5: BASELINE.json configs[3]; N = 8: configs[4]'s "draft x4 data-parallel"), whose tree round
    # (MQ_LEN / D rows per step) then hides behind the verify instead of lengthening rank 0's step.
    placement = args.placement
    if placement == "auto":
        placement = "dedicated" if (is_async and world >= 5) else "colocated"
    dedicated = is_async and placement == "dedicated" and world > 1
    if eagle and placement == "dedicated" and args.placement == "auto" and (world - 1) & (world - 2):
        placement = "colocated"         # the EAGLE draft is one rank: the target keeps a power-of-two degree only if N - 1 is one
    dedicated = is_async and placement == "dedicated" and world > 1
    if dedicated and eagle:
        ndraft = 1
    elif dedicated:
        ndraft = args.draft_dp if args.draft_dp > 0 else max(1, world - (1 << ((world - 1).bit_length() - 1)))
        ndraft = min(ndraft, world - 1)
    else:
        ndraft = 1
    tp = world - ndraft if dedicated else world
    assert tp >= 1 and tp & (tp - 1) == 0, f"target tensor-parallel degree {tp} must be a power of two" 
    kw = dict(hf_config=tcfg, draft=dname, draft_hf_config=dcfg, speculate=True, speculate_k=K, num_gpus=args.gpus,
              max_num_seqs=1, max_model_len=max_len, max_num_batched_tokens=max_len, kvcache_block_size=256,
              num_kvcache_blocks=blocks, num_draft_kvcache_blocks=blocks, enforce_eager=args.eager, weights_recipe=recipe)
    if is_async:
        kw.update(draft_async=True, async_fan_out=args.f, jit_speculate=True, inprocess_draft=not dedicated, num_draft_gpus=ndraft)
    if eagle:
        kw.update(use_eagle=True)
    guard.stage("engine_init")
    engine = LLMEngine(tname, **kw)
    if engine.is_draft_process:             # dedicated draft GPU: serve until the target says EXIT, then join the barrier
        guard.stage("draft_serve", guard.total_deadline)        # (waits for requests as long as the target runs)
        engine.serve()
        guard.stage("final_barrier", 120.0)
        dist.barrier()
        dist.destroy_process_group()
        return
    dev = engine.topo.device
    random.seed(0)
    prompt = [random.randint(0, 10000) for _ in range(args.input_len)]
    tp_group = engine.topo.tp_group

    def sync_all():
        torch.cuda.synchronize(dev)
        if tp > 1:
            dist.barrier(group=tp_group)
            torch.cuda.synchronize(dev)

    # ---- TTFT (chat.py:95-111 definition: generate() call -> first streamed token), p50 over a few runs ----
    guard.stage("ttft (first prefill + first speculation round: graph captures, first collectives in graphs)")
    ttfts, ttfts_round = [], []
    for _ in range(max(1, args.ttft_samples)):
        first = []
        sync_all()
        t0 = time.perf_counter()
        engine.generate([prompt], SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=1), use_tqdm=False,
                        stream_callback=lambda sid, toks: first.append(time.perf_counter()) if not first else None)
        ttfts.append((first[0] - t0) * 1e3)
        # the reference's loop hands the first token to the stream only after the first speculation round (the prefill's token
        # is appended at the start of that round): with max_new_tokens = 1 that is when generate() returns
        ttfts_round.append((time.perf_counter() - t0) * 1e3)
    # a prefill shape runs eagerly the first time and is captured the second time (engine/model_runner.py run): steady state
    # -- what a serving process sees for its recurring prompt shapes -- starts with the third sample
    kept = ttfts[2:] if len(ttfts) > 2 else ttfts[-1:]
    ttft_p50 = statistics.median(kept)
    # what a server with free-form prompt lengths sees: a shape on first sight runs eagerly (no graph yet).  Sample 0 above also
    # carries one-time costs of the process (first use of every kernel, allocator growth), so a FRESH shape is timed now that the
    # process is warm: a prompt one token shorter than any seen so far.
    ttft_first_sighting = None
    if args.full:
        guard.stage("ttft_first_sighting")
        first = []
        sync_all()
        t0 = time.perf_counter()
        engine.generate([prompt[:-1]], SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=1), use_tqdm=False,
                        stream_callback=lambda sid, toks: first.append(time.perf_counter()) if not first else None)
        ttft_first_sighting = (first[0] - t0) * 1e3
    ttft_round_p50 = statistics.median(ttfts_round[2:] if len(ttfts_round) > 2 else ttfts_round[-1:])

    # ---- timed decode steps through the real engine ----
    total = args.warmup + args.steps
    guard.stage("warmup_steps")
    engine.add_request(prompt, SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=total * (K + 1) + 8))
    for k_ in list(METRICS):
        METRICS[k_] = [] if isinstance(METRICS[k_], list) else 0
    step = engine.create_inference_step(engine.config)
    engine.step(step)                       # prefill
    for _ in range(args.warmup):
        engine.step(step)
    if not is_async and engine.draft_runner is not None:
        # synchronous speculation defers the draft's (K+1)-th, KV-deposit-only forward to the step after a fully accepted round:
        # its hipGraph would otherwise be captured (eager run + capture, tens of ms) by whichever TIMED step first needs it
        dr_ = engine.draft_runner
        with torch.inference_mode():
            dr_.d_slots[:1].fill_(-1)           # slot -1 = store nothing
            dr_._launch(("decode_deposit", 1), lambda: dr_._body_decode(1, False, head=False))
    n0 = len(METRICS["accepted_suffix_lens_with_recovery"])
    h0 = len(METRICS["cache_hits"])
    sync_all()
    guard.stage("timed_steps")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        engine.step(step)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if tp > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=tp_group)
        dt = float(t.item())
        dist.barrier(group=tp_group)
    lens = list(METRICS["accepted_suffix_lens_with_recovery"][n0:])
    hits = list(METRICS["cache_hits"][h0:])
    seq = engine.scheduler.running[0] if engine.scheduler.running else None
    ctx = len(seq) if seq is not None else args.input_len
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, seq, lens, hits)
    # ---- the reference's own protocol (bench/bench.py:34-51,233-235,351-352): random 128-token prompts, 512 output tokens,
    #      b = 1, temp 0; throughput = output tokens / wall clock of generate() (prefill included) and the decode-only rate
    #      (llm_engine.py:215-223).  Context grows 128 -> 640 here, where the timed steps above sit at ~130-300. ----
    ref = None
    if args.full and args.ref_seqs > 0:
        guard.stage("reference_protocol_run")
        engine.abort_all()                       # the timed request is not run to its end
        random.seed(1)
        rp = [[random.randint(0, 10000) for _ in range(args.input_len)] for _ in range(args.ref_seqs)]
        sync_all()
        t1 = time.perf_counter()
        outs, m = engine.generate(rp, SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=args.ref_output_len), use_tqdm=False)
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t1
        rl = m["accepted_suffix_lens_with_recovery"]
        rh = m["cache_hits"]
        ntok = sum(len(o["token_ids"]) for o in outs)
        ref = {"protocol": f"reference bench/bench.py: {args.ref_seqs} x ({args.input_len}-token random prompt -> {args.ref_output_len} output tokens), b=1, temp 0",
               "tokens_per_s_total": round(ntok / wall, 2),
               "tokens_per_s_decode": round(m["decode_total_tokens"] / m["decode_total_time"], 2) if m["decode_total_time"] else None,
               "mean_accepted_len": round(sum(rl) / max(1, len(rl)), 4),
               "cache_hit_rate": round(sum(rh) / len(rh), 4) if rh else None,
               "ms_per_step": round(1e3 * m["decode_total_time"] / max(1, len(rl)), 4), "final_context": args.input_len + args.ref_output_len,
               # the greedy stream is the TARGET's: independent of draft placement / data-parallelism at equal TP degree
               "stream_head": [int(t) for t in outs[0]["token_ids"][:48]]}
    tokens = sum(lens)
    ms_step = dt / args.steps * 1e3
    tm = engine.model_runner.model
    dr = engine.draft_runner                # None on ranks that do not host the draft
    # ---- the floor of tokens/s: the same steps with an INDEPENDENT draft (acceptance ~ 1 token per step, every async round a miss ->
    #      JIT chain on the critical path).  `value` above depends on how well the constructed pair agrees; this does not.  The draft's
    #      weight VALUES are overwritten in place (hipGraphs keep their pointers), the target is untouched. ----
    rand_pair = None
    if (args.full and recipe is not None and recipe.get("kind") == "pair" and dr is not None and not dedicated and tp == 1
            and not args.no_random_pair):
        guard.stage("random_pair_steps")
        from ssd_amd import weights as W
        engine.abort_all()
        with torch.inference_mode():
            dr.model.overwrite_weights(W.synthetic_weights(dcfg, 4242, 0.02, gen_device=str(dev), recipe=None))
        engine.add_request(prompt, SamplingParams(temperature=0, ignore_eos=True, max_new_tokens=(args.warmup + args.steps) * (K + 1) + 8))
        step_r = engine.create_inference_step(engine.config)
        engine.step(step_r)                 # prefill
        for _ in range(max(2, args.warmup)):
            engine.step(step_r)
        n1, h1 = len(METRICS["accepted_suffix_lens_with_recovery"]), len(METRICS["cache_hits"])
        sync_all()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            engine.step(step_r)
        torch.cuda.synchronize(dev)
        dtr = time.perf_counter() - t1
        lr, hr = METRICS["accepted_suffix_lens_with_recovery"][n1:], METRICS["cache_hits"][h1:]
        rand_pair = {"tokens_per_s": round(sum(lr) / dtr, 3), "ms_per_step": round(dtr / args.steps * 1e3, 4),
                     "mean_accepted_len": round(sum(lr) / max(1, len(lr)), 4), "cache_hit_rate": round(sum(hr) / len(hr), 4) if hr else None,
                     "draft": "independent N(0, 0.02) weights written over the pair's draft in place (same graphs, same shapes)"}
        engine.abort_all()
    tb = tm.weight_bytes()
    kv_tok = lambda m: 2 * m.cfg.num_layers * m.nkv * m.hd * 2
    hit_rate = sum(hits) / len(hits) if hits else None
    if is_async:
        # per round the draft GPU runs: glue (K+1 rows) + K tree steps (MQ_LEN rows) -- off the critical path when the
        # request hits the speculation cache -- plus, on a miss, the K-forward JIT chain on the critical path
        miss = 1.0 - (hit_rate or 0.0)
        draft_fwd = 1 + K + miss * K
        legs = [(engine.model_runner, K + 1, 1), (dr, K + 1, 1), (dr, engine.config.MQ_LEN, K), (dr, 1, miss * K)]
        if eagle:       # the one-layer EAGLE draft has its own launch list (ssd_amd/eagle.py): the GEMM roofline covers the target
            legs = legs[:1]
    else:
        # K chained forwards + the deferred KV-deposit forward, which only follows a fully accepted round
        draft_fwd = K + sum(1 for n in lens if n == K + 1) / max(1, len(lens))
        legs = [(engine.model_runner, K + 1, 1), (dr, 1, draft_fwd)]
    db = dr.model.weight_bytes() if dr is not None else 0
    dkv = kv_tok(dr.model) if dr is not None else 0
    colocated_bytes = 0 if (dedicated or dr is None) else draft_fwd * (db + ctx * dkv)
    step_bytes = tb + ctx * kv_tok(tm) + colocated_bytes      # HBM bytes THIS GPU (TP rank 0) streams per step
    mode = (f"async SSD k={K} f={args.f} ({'dedicated draft GPU, RCCL p2p' if dedicated else 'draft co-located on TP rank 0'}, jit backup)"
            if is_async else f"sync speculative decoding k={K} (draft replicated)")
    out = {
        "metric": ("output tokens/sec + p50 TTFT, Llama-3-70B SSD k=7 f=3; mean accepted len" if args.workload == "c4" and K == 7 and args.f == 3
                   else "output tokens/sec (speculative decoding, b=1, temp 0), with p50 TTFT and mean accepted length"),
        "value": round(tokens / dt, 3), "unit": "tokens/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_step, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic token ids (random.seed(0), randint(0,10000)) + synthetic seeded weights "
                + ("(peaky recipe: the LM-head rows of the same 3 tokens scaled x6 in the target and in its EAGLE-3 draft, so that they agree now and then)"
                   if (recipe and eagle and recipe["kind"] == "peaky") else
                   f"(constructed EAGLE pair, snr {args.pair_snr}: a correlated-pair target whose head favours the draft vocabulary + a draft wired to compute the target's token map)"
                   if (recipe and eagle) else
                   f"(correlated-pair recipe, snr {args.pair_snr}, layer_gain {recipe['layer_gain']}: real shapes, values built so draft and target "
                   f"mostly agree -- shared embedding / head base vectors, o_proj and down_proj scaled by layer_gain so the decoder layers "
                   f"perturb the residual stream instead of drowning it; every matrix is streamed in full)"
                   if recipe else "(independent N(0,0.02): acceptance ~0)"),
        "config": {"workload": f"{args.workload}: {tname} target TP={tp} + {dname} draft, {mode}, b=1, temp=0, "
                               f"input_len={args.input_len}, kv block 256, max_model_len {max_len}",
                   "parallelism": f"tp{tp}" + (f"+draft{ndraft}" if dedicated else ""), "hipgraph": not args.eager,
                   "pair": (("peaky" if recipe["kind"] == "peaky" else "constructed") if recipe else "random") if eagle else args.pair, "eagle3": eagle,
                   "parity": "greedy token streams bit-exact vs the reference-driven traces up to recorded near-ties (top-2 margin <= 1 bf16 "
                             "ulp); the north_star's '1e-3 abs on verify logits' is enforced on the fp32 LM-head epilogue and, at model "
                             "level, as rms|HIP - fp64 truth| <= 1.25 x rms|reference - fp64 truth| + 1e-3 (two bf16 pipelines cannot "
                             "agree to 1e-3: one bf16 ulp at |logit| 8 is 0.0625) -- tests/test_real_shapes_gpu.py, DESIGN.md section 5"},
        "mean_accepted_len": round(tokens / max(1, len(lens)), 4),
        "cache_hit_rate": None if hit_rate is None else round(hit_rate, 4),
        "ttft_p50_ms": round(ttft_p50, 3), "ttft_samples_ms": [round(t, 2) for t in kept],
        # TTFT = generate() call -> first token at the stream callback (reference bench/chat.py:95-111).  This engine streams the
        # prefill's token when the prefill returns; the reference's loop (and this repo until round 2) streams it one speculation
        # round later -- that figure is kept beside it
        "ttft_after_first_round_p50_ms": round(ttft_round_p50, 3),
        # eager prefill of a prompt length met for the first time (warm process); `ttft_cold_process_ms` = the very first request
        "ttft_first_sighting_ms": None if ttft_first_sighting is None else round(ttft_first_sighting, 3),
        "ttft_cold_process_ms": round(ttfts[0], 3),
        # the reference's own protocol (2 x 128 -> 512 tokens, prefill included, context -> 640): THE tokens/s to quote
        "value_reference_protocol": None if ref is None else ref["tokens_per_s_total"],
        # the floor: the same engine and step with an independent draft (mean accepted length ~ 1): tokens/s that does not depend on the pair
        "value_random_pair": None if rand_pair is None else rand_pair["tokens_per_s"], "random_pair": rand_pair,
        "draft_forwards_per_step": round(draft_fwd, 3),
        "step_hbm_bytes_per_gpu": int(step_bytes),
        "step_roofline_frac": round(step_bytes / (dt / args.steps) / HBM_PEAK, 4),
        # the same without the bytes of the co-located draft: target weights + target KV only (what a dedicated-draft layout streams)
        "step_roofline_frac_target_only": round((tb + ctx * kv_tok(tm)) / (dt / args.steps) / HBM_PEAK, 4),
        "tokens_per_s_at_accepted_len": {str(a): round(a / (dt / args.steps), 1) for a in (1, 2, 4, K + 1)},
        "reference_protocol": ref,
    }
    if not args.full:                 # measured by --full only: a plain line does not carry them
        for k_ in ("ttft_first_sighting_ms", "value_reference_protocol", "value_random_pair", "random_pair", "reference_protocol"):
            del out[k_]
    if world > 1:                     # first contact with a multi-GPU box: say up front which transport carries the sums and how far the
        # first-run paths of DESIGN.md section 7 got (a failure record carries the same two fields)
        out = {"collective_one_shot_status": getattr(engine.model_runner, "custom_ar_status", None),
               "first_run_paths": guard.first_run_paths(), **out}
        if rank == 0:
            print(f"[ssd bench] n_gpus {world}: one-shot all-reduce: {out['collective_one_shot_status']}; first-run paths completed: "
                  f"{out['first_run_paths']['completed']}", file=sys.stderr, flush=True)
    if args.full and not args.no_roofline:          # every rank launches the same sequence (shard shapes); rank 0 reports
        guard.stage("roofline_probe")
        with torch.inference_mode():      # the engine's buffers are inference tensors (ModelRunner runs under inference_mode)
            roof = gemm_roofline(legs)
            if tp > 1:
                out["collective"] = collective_probe(engine, K + 1)
        out["roofline"] = roof
    if rank == 0:
        if args.full and not args.no_cpu_baseline:
            guard.stage("cpu_baseline")
            try:
                out["cpu_baseline"] = cpu_baseline()
            except Exception as e:  # the baseline must never take the GPU number down with it
                out["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": os.cpu_count(), "kind": "port",
                                       "sample": f"failed: {e!r}"}
        print(json.dumps(out), flush=True)
    guard.done()                            # the line is out: nothing after this may replace it with a failure record
    engine.exit()                           # dedicated placement: tells the draft rank to leave its serve loop
    if world > 1:
        # bounded farewell: a rank that is gone must not keep the others in the barrier / in a communicator destructor
        import threading
        threading.Timer(90.0, lambda: os._exit(0 if rank == 0 else 5)).start()
        dist.barrier()
        dist.destroy_process_group()
        os._exit(0)


if __name__ == "__main__":
    main()
