"""A Qwen3-MoE target end to end on the MI355X: model logits against float64 truth with the decoder's own routes forced (bar, as in
tests/test_kv8_engine_gpu.py: rms|HIP - truth| <= 1.25 rms|bf16 pipeline - truth| + 1e-3 over all logits, the same argmax outside
near-ties), the routes being the decoder's own top-k of its own bf16 router logits; equal greedy streams in the three decoding
modes; graph replays against eager runs; the dense path left as it was; memory accounting; a 300-token prefill.

The pair: tests/moe_ref.tiny_moe_config (2 layers, h 128, 8 experts, top 2: the configuration of tests/test_moe_cpu.py) with
router_gain 8 as target, a 2-layer dense Qwen3 of the same vocabulary as draft -- both with head_dim 64 instead of the CPU test's 32:
the engine's RoPE / KV-store and attention kernels, which this family leaves untouched, take head_dim 64, 128 or 256 only.  SEED was chosen on the CPU with moe_ref's bf16 pipeline alone: over the 8-token prompt and the 24 greedy
tokens that pipeline generates, every k-th / (k+1)-th router-logit margin is at least MIN_ULPS bf16 ulps of the larger value (the
stream test asserts the same of the decoder's own trace, as an input condition)."""
import gc
import json
import os

import pytest
import torch

from tests import moe_ref as R
from tests.util import NEAR_TIE

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED, GAIN, STD = 158, 8.0, 0.1
MIN_ULPS = 4
PROMPT = [(29 * i + 5) % 512 for i in range(8)]
ENGINE_KW = dict(max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)
_W = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _pair():
    """(target config, target weights, draft config, draft weights): generated once, never modified."""
    if not _W:
        from ssd_amd import weights as W
        from ssd_amd.model_config import ModelConfig
        t = R.tiny_moe_config(head_dim=64)
        d = ModelConfig("qwen3", 128, 2, 4, 2, 64, 256, 512, 1e-6, 1e6, 1024, True, True)
        _W["pair"] = (t, W.synthetic_state_dict(t, seed=SEED, std=STD, recipe={"router_gain": GAIN}),
                      d, W.synthetic_state_dict(d, seed=SEED + 1, std=STD))
    return _W["pair"]


def _decoder(cfg, w, gpu, max_tokens, nblocks, bs=16):
    from ssd_amd.model import HipDecoder
    dec = HipDecoder(cfg, max_tokens=max_tokens, max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=max(512, max_tokens + 16),
                     device=gpu)
    dec.load_weights(iter(w.items()))
    dec.alloc_kv(nblocks)
    return dec


def _hip_rows(dec, tokens, chunks, gpu, bs=16):
    """Eager forwards over `tokens` cut into `chunks` (the first a prefill, the rest cached decode / verify rows) with moe_trace on
    -> (logits float64 [T, V], per layer router logits [T, E], per layer topk ids [T, k])."""
    from ssd_amd.hip import ops as H
    from ssd_amd.model import AttnMeta
    T = len(tokens)
    nblocks = -(-T // bs) + 1
    table = list(range(nblocks))
    bt = torch.tensor([table], dtype=torch.int32, device=gpu)
    sl = lambda ps: torch.tensor([table[p // bs] * bs + p % bs for p in ps], dtype=torch.int32, device=gpu)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=gpu)
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device=gpu)
    L = dec.cfg.num_layers
    dec.moe_trace = []
    rows, p0 = [], 0
    for n in chunks:
        p1 = p0 + n
        if p0 == 0:
            meta = AttnMeta(H.MODE_CAUSAL, 1, n, sl(range(n)), i32([n]), bt, cu_q=i32([0, n]))
        else:
            meta = AttnMeta(H.MODE_CAUSAL, 1, n, sl(range(p0, p1)), i32([p1]), bt, q_per_seq=n)
        dec.forward(i64(tokens[p0:p1]), i64(range(p0, p1)), n, meta)
        m = dec.compute_logits(n)
        rows.append(dec.logits[:m].double().cpu())
        p0 = p1
    assert p0 == T and len(dec.moe_trace) == L * len(chunks)
    trace, dec.moe_trace = dec.moe_trace, None
    rl = [torch.cat([trace[c * L + li][0] for c in range(len(chunks))]) for li in range(L)]
    ids = [torch.cat([trace[c * L + li][1] for c in range(len(chunks))]) for li in range(L)]
    return torch.cat(rows), rl, ids


def _assert_forced_route_bar(cfg, w, tokens, got, rl, ids, what):
    k = cfg.num_experts_per_tok
    for li in range(cfg.num_layers):
        assert rl[li].dtype == BF and rl[li].shape == (len(tokens), cfg.num_experts)
        assert torch.equal(R.topk_ids(rl[li], k), ids[li].long()), f"{what}: layer {li} routes are not the top-k of the decoder's own logits"
    truth, _, _ = R.forward(cfg, w, tokens, forced_routes=ids)
    pipe, _, _ = R.forward(cfg, w, tokens, pipeline=True, forced_routes=ids)
    e_hip, e_ref = (got - truth).abs(), (pipe - truth).abs()
    r_hip, r_ref = e_hip.pow(2).mean().sqrt().item(), e_ref.pow(2).mean().sqrt().item()
    d_max = (got - pipe).abs().max().item()
    print(f"{what}: rms|HIP-truth| {r_hip:.5f} (max {e_hip.max():.4f}) | rms|bf16 pipeline-truth| {r_ref:.5f} (max {e_ref.max():.4f}) | "
          f"max|HIP-pipeline| {d_max:.4f}")
    assert torch.isfinite(got).all()
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: rms |HIP - truth| {r_hip:.5f} > 1.25 x {r_ref:.5f} + 1e-3"
    top2 = pipe.topk(2, dim=-1).values
    thr = max(NEAR_TIE, 2 * d_max)
    assert bool(((got.argmax(-1) == pipe.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all()), f"{what}: argmax differs beyond a near-tie"


def test_forced_route_logits_prefill_decode_verify(gpu):
    cfg, w, _, _ = _pair()
    tokens = [(37 * i + 11) % 512 for i in range(24 + 6 + 8)]
    dec = _decoder(cfg, w, gpu, 64, 4)
    assert dec.moe and not (dec.use_parts or dec.fuse_attn_o or dec.pf_parts or dec.chain_seg or dec.tree_seg)
    assert all(dec.fusion_plan(T) == (False, False) for T in (1, 8, 16, 24))
    assert dec.moe_trace is None
    got, rl, ids = _hip_rows(dec, tokens, [24] + [1] * 6 + [8], gpu)
    _assert_forced_route_bar(cfg, w, tokens, got, rl, ids, "tiny MoE prefill 24 + 6 decode + verify 8")


def test_300_token_prefill(gpu):
    """Long enough for the long-prefill GEMM of the dense linears and many row tiles per expert (75 rows each on average)."""
    cfg, w, _, _ = _pair()
    tokens = [(53 * i + 7) % 512 for i in range(300)]
    dec = _decoder(cfg, w, gpu, 320, 21)
    got, rl, ids = _hip_rows(dec, tokens, [300], gpu)
    counts = torch.bincount(ids[0].reshape(-1), minlength=cfg.num_experts)
    assert int(counts.max()) > 64, "input problem: no expert with more than one 64-row pass"
    _assert_forced_route_bar(cfg, w, tokens, got, rl, ids, "tiny MoE prefill 300")


def _factory(wt, wd):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter((wd if is_draft else wt).items()), **kw)
    return f


def _engine(mode, eager=False, **extra):
    from ssd_amd.engine.llm_engine import LLMEngine
    t, wt, d, wd = _pair()
    kw = dict(ENGINE_KW, hf_config=t, runner_factory=_factory(wt, wd), enforce_eager=eager, **extra)
    if mode != "ar":
        kw.update(draft="d", draft_hf_config=d, speculate=True, speculate_k=3)
    if mode == "async":
        kw.update(draft_async=True, async_fan_out=2, jit_speculate=True, inprocess_draft=True)
    return LLMEngine("moe", **kw)


def _generate(mode, eager=False, trace=False, n=24):
    from ssd_amd.sampling_params import SamplingParams
    eng = _engine(mode, eager)
    assert eng.model_runner.model.moe and (eng.draft_runner is None or not eng.draft_runner.model.moe)
    eng.model_runner.margin_log = {}
    if trace:
        eng.model_runner.model.moe_trace = []
    out, _ = eng.generate([PROMPT], SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True), use_tqdm=False)
    res = dict(tokens=out[0]["token_ids"], margins=dict(eng.model_runner.margin_log), trace=eng.model_runner.model.moe_trace,
               graphs=sorted({k[0] for k in eng.model_runner.graphs}))
    eng.exit()
    del eng
    gc.collect()
    return res


@pytest.fixture(scope="module")
def ar_eager(gpu):
    """The autoregressive run, eager with moe_trace on: the stream every other mode is compared with, and the input condition."""
    return _generate("ar", eager=True, trace=True)


def test_streams_equal_in_three_modes(gpu, ar_eager):
    from tests.util import assert_stream_matches, seq_margins
    cfg = _pair()[0]
    k = cfg.num_experts_per_tok
    assert len(ar_eager["tokens"]) == 24 and len(ar_eager["trace"]) >= cfg.num_layers * 24
    worst = float("inf")
    for logits, ids in ar_eager["trace"]:
        assert torch.equal(R.topk_ids(logits, k), ids.long())
        margin, big = R.kth_margins(logits, k)
        worst = min(worst, float((margin / R.bf16_ulp(big)).min()))
    print(f"autoregressive trace: smallest k-th / (k+1)-th router margin {worst:.2f} bf16 ulps of the larger value")
    assert worst >= MIN_ULPS, f"input problem, not a product failure: a routing margin of {worst:.2f} ulps < {MIN_ULPS} (choose another SEED)"
    margins = seq_margins(ar_eager["margins"], 0)
    for mode in ("sync", "async"):
        got = _generate(mode)
        n = assert_stream_matches(got["tokens"], ar_eager["tokens"], margins, len(PROMPT), what=f"MoE target {mode} vs autoregressive")
        print(f"MoE target {mode}: {n} of 24 tokens identical to the autoregressive stream; graphs {got['graphs']}")


@pytest.mark.parametrize("mode", ["ar", "sync"])
def test_graph_replays_give_the_eager_tokens(gpu, ar_eager, mode):
    from tests.util import assert_stream_matches, seq_margins
    eager = ar_eager if mode == "ar" else _generate(mode, eager=True)
    graph = _generate(mode)
    assert eager["graphs"] == [] and any(g.startswith("decode") or g.startswith("verify") for g in graph["graphs"]), graph["graphs"]
    assert graph["tokens"] == eager["tokens"], f"{mode}: the graph replays and the eager launches are the same kernels on the same inputs"
    assert_stream_matches(graph["tokens"], ar_eager["tokens"], seq_margins(ar_eager["margins"], 0), len(PROMPT), what=f"{mode} graphs")


@pytest.mark.parametrize("mode", ["ar", "sync"])
def test_dense_model_launches_what_it_launched_before(gpu, monkeypatch, mode):
    """A dense model with every MoE code path patched out (the entry points and the decoder's MoE methods raise) makes the ordered
    calls and creates the graphs that tests/golden/launch_trace.json recorded before this family existed."""
    from ssd_amd.hip import moe_ops
    from ssd_amd.model import HipDecoder
    from tests.test_launch_trace_gpu import FIXTURE, run_scenario
    with open(FIXTURE) as f:
        recorded = json.load(f)

    def boom(*a, **k):
        raise AssertionError("a dense model reached a MoE code path")
    name = f"{mode}-greedy"
    want = recorded["scenarios"][name]
    runs = []
    for eager in (True, False):          # (a context each: the recorder of the eager run is undone before the graph run starts)
        with monkeypatch.context() as mp:
            for fn in ("moe_route", "moe_gemm", "moe_combine", "load_moe_library"):
                mp.setattr(moe_ops, fn, boom)
            for fn in ("_alloc_moe", "_load_moe", "_moe_up", "_moe_down"):
                mp.setattr(HipDecoder, fn, boom)
            runs.append(run_scenario(name, eager, mp.setattr))
    got, graphs = runs
    assert got["trace"] == [recorded["entries"][i] for i in want["trace"]]
    assert graphs["graphs"] == want["graphs"]
    if want["eager_tokens"] is not None:
        assert got["tokens"] == want["eager_tokens"]
    if want["graph_tokens"] is not None:
        assert graphs["tokens"] == want["graph_tokens"]


def test_weight_bytes_and_auto_sized_kv_cache(gpu, monkeypatch):
    from ssd_amd.engine.llm_engine import LLMEngine
    t, wt, _, _ = _pair()
    seen = []
    real = torch.cuda.mem_get_info

    def spy(*a, **k):
        free, total = real(*a, **k)
        seen.append(free)
        return free, total
    monkeypatch.setattr(torch.cuda, "mem_get_info", spy)
    kw = dict(ENGINE_KW, num_kvcache_blocks=-1, gpu_memory_utilization=0.01)
    eng = LLMEngine("moe", hf_config=t, runner_factory=_factory(wt, None), **kw)
    m = eng.model_runner.model
    E, I, h, L = t.num_experts, t.moe_intermediate_size, t.hidden_size, t.num_layers
    tables = {n: v for n, v in m.w.items() if ".mlp." in n}
    assert len(tables) == 3 * L
    per_layer = (16 * h + E * 2 * I * h + E * h * I) * 2            # the router padded to 16 rows, gate_up, down: bf16
    assert sum(v.numel() * v.element_size() for v in tables.values()) == L * per_layer
    assert m.weight_bytes() == sum(v.numel() * v.element_size() for n, v in m.w.items() if n != "model.embed_tokens.weight")
    assert m.weight_bytes() > L * per_layer
    # the cache was sized from the memory that was free AFTER the tables (and the act / d buffers) existed
    assert seen and eng.model_runner.num_kvcache_blocks == int(seen[-1] * 0.01) // m.kv_block_bytes()
    assert m.kv_cache.shape[2] == eng.model_runner.num_kvcache_blocks
    assert m.moe_act.shape == (512 * t.num_experts_per_tok, I) and m.moe_d.shape == (512 * t.num_experts_per_tok, h)
    eng.exit()
