"""LoRA adapters end to end on the MI355X: decoder logits against float64 arithmetic on the merged weights W + scale * B . A (bar:
rms|HIP - f64| <= 1.25 rms|oracle - f64| + 1e-3 over a prefill plus an 8-row verify, the oracle being the unmodified CPU oracle on the
merged weights rounded to bf16), a zero-B adapter against the base rows route, greedy engine streams in lock step with the oracle
engine on merged weights (sync and async speculation, the adapter on the target only), a mixed batch on the base and two adapters
with shared prefixes and preemption, the prefix cache's adapter roots, the adapter lifecycle, and the default path's launches.

Adapter recipe (tests/lora_ref.make_adapter): r = 8, alpha = 16 on all seven modules, A ~ N(0, 1/K), B ~ N(0, 0.02^2), one
torch.Generator drawn in layer order, module order, A before B, rounded to bf16.  The seed of the lock-step runs is chosen on the CPU
so that the oracle's own run has at most 4 of its 24 decisions at a margin <= 0.0625 (seed 12: 4; only 1 of its 24 tokens equals the
base model's): the reference alone then stays within the cap of the comparison even if every near-tie flipped."""
import dataclasses
import random

import pytest
import torch

from tests import lora_ref as LR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED = 12


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _adapter(cfg, seed, r=8, alpha=16, **kw):
    from ssd_amd.lora import module_shapes
    return LR.make_adapter(module_shapes(cfg), cfg.num_layers, r, alpha, seed, **kw)


def _run_hip(cfg, w, adapter, seq, n_verify, gpu, slot_rows, max_rank=16, **dec_kw):
    """Prefill of seq[:-n_verify] then one verify forward of n_verify rows on a decoder with two adapter slots, `adapter` in slot 1;
    slot_rows: the slot every row names (1, or -1 for the base on the rows route).  -> (logits float64 [T, V], the decoder)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.lora import load_adapter
    from ssd_amd.model import HipDecoder, AttnMeta
    P, T = len(seq) - n_verify, len(seq)
    bs = 16
    nblocks = -(-T // bs) + 1
    dec = HipDecoder(cfg, max_tokens=max(T, 64), max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=max(512, T + 16),
                     device=gpu, max_loras=2, max_lora_rank=max_rank, **dec_kw)
    ws = dict(w)
    if cfg.tie_word_embeddings:
        ws.pop("lm_head.weight", None)
    dec.load_weights(iter(ws.items()))
    dec.alloc_kv(nblocks)
    dec.set_lora(1, load_adapter(adapter, cfg, max_rank))
    dec.lora_rows.fill_(slot_rows)
    dec.lora_active = True
    table = list(range(nblocks))
    bt = torch.tensor([table], dtype=torch.int32, device=gpu)
    sl = lambda ps: torch.tensor([table[p // bs] * bs + p % bs for p in ps], dtype=torch.int32, device=gpu)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=gpu)
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device=gpu)
    dec.forward(i64(seq[:P]), i64(range(P)), P, AttnMeta(H.MODE_CAUSAL, 1, P, sl(range(P)), i32([P]), bt, cu_q=i32([0, P])))
    n = dec.compute_logits(P)
    got_p = dec.logits[:n].clone()
    dec.forward(i64(seq[P:]), i64(range(P, T)), n_verify,
                AttnMeta(H.MODE_CAUSAL, 1, n_verify, sl(range(P, T)), i32([T]), bt, q_per_seq=n_verify))
    n = dec.compute_logits(n_verify)
    return torch.cat([got_p, dec.logits[:n]]).cpu(), dec


def _logits_vs_truth(cfg, w, prompt, n_verify, gpu, what, seed=1, r=8, max_rank=16, quantization=None, kv8=False):
    from oracle.model import OracleModel, Ctx
    from tests.util import truth_forward
    w_base64 = w
    if quantization == "w4a16":
        from tests.test_w4a16_engine_gpu import quantized
        w_base64 = quantized(w)[1]                  # the exact s * q the int4 target computes with
    adapter = _adapter(cfg, seed, r=r)
    w_orc, w_truth = LR.merge_state_dict(w_base64, adapter, cfg.num_layers)
    seq = list(prompt)
    T = len(seq)
    dec_kw = dict(quantization=quantization) if quantization else {}
    if kv8:
        dec_kw["kv_cache_dtype"] = "fp8"
    got_bf, dec = _run_hip(cfg, w, adapter, seq, n_verify, gpu, 1, max_rank=max_rank, **dec_kw)
    got = got_bf.double()
    strip = lambda d: {k: v for k, v in d.items() if not (cfg.tie_word_embeddings and k == "lm_head.weight")}
    bs, nblocks = 16, -(-T // 16) + 1
    table = list(range(nblocks))
    cu = torch.tensor([0, T], dtype=torch.int32)
    ctx = Ctx("prefill", slot_mapping=torch.tensor([table[p // bs] * bs + p % bs for p in range(T)], dtype=torch.int32), cu_q=cu, cu_k=cu)
    if kv8:
        from tests import kv8_ref
        orc = kv8_ref.Kv8OracleModel(cfg, strip(w_orc), nblocks, bs)
        orc.set_kv_scales(None, None)
        truth = kv8_ref.truth_forward_kv8(cfg, strip(w_truth), seq, None, None)
        base_truth = kv8_ref.truth_forward_kv8(cfg, strip(w_base64), seq, None, None)
    else:
        orc = OracleModel(cfg, strip(w_orc), nblocks, bs)
        truth = truth_forward(cfg, strip(w_truth), seq)
        base_truth = truth_forward(cfg, strip(w_base64), seq)
    ref_h = orc.forward(torch.tensor(seq), torch.arange(T), ctx)
    ref_h = ref_h[0] if isinstance(ref_h, tuple) else ref_h
    ref = orc.compute_logits(ref_h).double()
    rms = lambda e: e.pow(2).mean().sqrt().item()
    r_hip, r_ref, r_base = rms(got - truth), rms(ref - truth), rms(base_truth - truth)
    bar = 1.25 * r_ref + 1e-3
    print(f"{what}: rms|HIP-f64| {r_hip:.5f} | rms|oracle-f64| {r_ref:.5f} | bar {bar:.5f} | rms|base f64 - adapted f64| {r_base:.5f}")
    assert torch.isfinite(got).all()
    assert r_base > 10 * bar, f"{what}: the adapter moves the truth by {r_base:.5f}, not more than ten bars ({bar:.5f}): the case shows nothing"
    assert r_hip <= bar, f"{what}: rms |HIP - f64| {r_hip:.5f} > 1.25 x {r_ref:.5f} + 1e-3"
    return dec


def _golden_model(golden, name):
    from tests.test_model_gpu import mk_cfg
    g = golden(name)
    cfg = mk_cfg(g, "qwen3", tie=True, qk_norm=True) if name == "tiny_qwen3" else mk_cfg(g, "llama")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    return cfg, w, g["prompt"].tolist() + g["verify_tokens"].tolist(), len(g["verify_tokens"])


def test_tiny_llama_lora_logits(gpu, golden):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_llama")
    dec = _logits_vs_truth(cfg, w, prompt, nv, gpu, "tiny llama lora")
    assert dec.max_loras == 2 and dec.lora_geo["qkv"][2] == 64 and dec.lora_geo["o"][2] == 32 and dec.lora_bytes() > 0


def test_tiny_qwen3_lora_logits(gpu, golden):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_qwen3")
    _logits_vs_truth(cfg, w, prompt, nv, gpu, "tiny qwen3 lora", max_rank=64)


def test_300_row_prompt_lora_logits(gpu):
    """308 rows: every linear is one long-prefill GEMM launch, the shrink keeps one slab."""
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    w = W.synthetic_state_dict(cfg, seed=7, std=0.05)
    random.seed(5)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(308)]
    assert 300 > HipDecoder.LORA_SPLIT_MAX_T and HipDecoder._lm_eligible(300)
    _logits_vs_truth(cfg, w, prompt, 8, gpu, "300-row prompt lora")


def test_two_layer_70b_cut_rank16_lora_logits(gpu):
    from ssd_amd import weights as W
    from ssd_amd.model_config import PRESETS
    cfg = dataclasses.replace(PRESETS["llama-3.1-70b"], num_layers=2, vocab_size=4096)
    w = W.synthetic_state_dict(cfg, seed=4, std=0.02)
    random.seed(3)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(24)]
    _logits_vs_truth(cfg, w, prompt, 8, gpu, "70B x 2 layers lora r16", r=16, max_rank=16)


def test_tiny_llama_w4a16_lora_logits(gpu, golden):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_llama")
    dec = _logits_vs_truth(cfg, w, prompt, nv, gpu, "tiny llama w4a16 + lora", quantization="w4a16")
    assert dec.w4


def test_tiny_llama_kv8_lora_logits(gpu, golden):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_llama")
    dec = _logits_vs_truth(cfg, w, prompt, nv, gpu, "tiny llama fp8 KV + lora", kv8=True)
    assert dec.kv8


@pytest.mark.parametrize("model", ["tiny_llama", "tiny_qwen3"])
def test_zero_b_adapter_reproduces_the_base_rows_route(gpu, golden, model):
    """B = 0: y = bf16(y0 + scale * 0).  Both runs take the rows route (lora_active), one with every row on the adapter, one with
    every row on no adapter; 1 bf16 ulp."""
    from tests.util import ulp_stats
    cfg, w, prompt, nv = _golden_model(golden, model)
    adapter = _adapter(cfg, 3, zero_b=True)
    on, _ = _run_hip(cfg, w, adapter, prompt, nv, gpu, 1)
    off, _ = _run_hip(cfg, w, adapter, prompt, nv, gpu, -1)
    mx, frac = ulp_stats(on, off)
    print(f"{model} zero-B: max ulp {mx}, fraction differing {frac:.5f}")
    assert mx <= 1


# ---------------------------------------------------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------------------------------------------------
def _factory(w):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(w[is_draft].items()), **kw)
    return f


def _oracle_without_lora(eng):
    """The oracle engine runs MERGED weights: it is handed the same requests with the adapter's name taken off."""
    from ssd_amd.engine.llm_engine import LLMEngine
    eng.add_request = lambda prompt, sp: LLMEngine.add_request(eng, prompt, dataclasses.replace(sp, lora=None))
    return eng


def _engine_golden(golden):
    from tests.test_model_gpu import mk_cfg, weights
    g = golden("engine_golden")
    return g, mk_cfg(g, "llama", "t_"), mk_cfg(g, "llama", "d_"), weights(g, "t."), weights(g, "d.")


_OWN = {}


def _oracle_own_run(golden):
    """The oracle target's own greedy run of 24 tokens on the merged weights (autoregressive: the target's decisions are the same
    under every speculation mode): (decisions at a margin <= 0.0625, its tokens, the base model's tokens)."""
    if not _OWN:
        from oracle.runner import oracle_runner_factory
        from ssd_amd.engine.llm_engine import LLMEngine
        from ssd_amd.sampling_params import SamplingParams
        g, tc, dc, wt, wd = _engine_golden(golden)
        merged = LR.merge_state_dict(wt, _adapter(tc, SEED), tc.num_layers)[0]
        prompt = g["prompt"].tolist()
        kw = dict(hf_config=tc, max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64)
        sp = SamplingParams(temperature=0, max_new_tokens=24, ignore_eos=True)
        own = LLMEngine("t", runner_factory=oracle_runner_factory(merged), **kw)
        own.model_runner.margin_log = {}
        toks = own.generate([prompt], sp, use_tqdm=False)[0][0]["token_ids"]
        margins = {pos: m for (_, pos), m in own.model_runner.margin_log.items() if len(prompt) <= pos < len(prompt) + 24}
        assert len(margins) == 24, sorted(margins)
        base = LLMEngine("t", runner_factory=oracle_runner_factory(wt), **kw).generate([prompt], sp, use_tqdm=False)[0][0]["token_ids"]
        _OWN["r"] = (sum(m <= 0.0625 for m in margins.values()), toks, base)
    return _OWN["r"]


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_lora_target_engine_lockstep_with_oracle(gpu, golden, mode):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.utils.topology import Topology
    from tests.lockstep import compare_lockstep
    g, tc, dc, wt, wd = _engine_golden(golden)
    adapter = _adapter(tc, SEED)
    merged = LR.merge_state_dict(wt, adapter, tc.num_layers)[0]
    kw = dict(hf_config=tc, draft="d", draft_hf_config=dc, speculate=True, max_model_len=512, max_num_batched_tokens=512,
              kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)
    if mode == "async":
        kw.update(speculate_k=3, draft_async=True, async_fan_out=2, jit_speculate=True)
    else:
        kw.update(speculate_k=int(g["sd_K"]))
    prompt = g["prompt"].tolist()
    cpu_kw = dict(inprocess_draft=mode == "async", topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    near, own_toks, base_toks = _oracle_own_run(golden)
    print(f"lora target {mode}: the oracle's own run has {near} of 24 decisions at a margin <= 0.0625")
    assert near <= 4 and own_toks != base_toks

    gpu_eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), inprocess_draft=mode == "async", enable_lora=True,
                        max_loras=2, max_lora_rank=16, **kw)
    gpu_eng.add_lora("x", adapter)
    assert gpu_eng.list_loras() == ["x"]
    cpu_eng = _oracle_without_lora(LLMEngine("t", runner_factory=oracle_runner_factory(merged, wd), **cpu_kw))
    rep = compare_lockstep(gpu_eng, cpu_eng, prompt, 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True, lora="x"),
                           fan_out=2 if mode == "async" else None, what=f"lora target {mode}")
    print(f"lora target {mode}: {rep.summary()}")
    assert any(k[0].endswith("_a") for k in gpu_eng.model_runner.graphs), sorted({k[0] for k in gpu_eng.model_runner.graphs})
    assert gpu_eng.draft_runner is None or not any(k[0].endswith("_a") for k in gpu_eng.draft_runner.graphs)
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()
    # the adapted greedy stream differs from the base stream of the same engine
    ad, _ = gpu_eng.generate([prompt], SamplingParams(temperature=0, max_new_tokens=24, ignore_eos=True, lora="x"), use_tqdm=False)
    ba, _ = gpu_eng.generate([prompt], SamplingParams(temperature=0, max_new_tokens=24, ignore_eos=True), use_tqdm=False)
    assert ad[0]["token_ids"] != ba[0]["token_ids"]
    gpu_eng.exit()


def _small_models():
    from ssd_amd import weights as W
    from ssd_amd.model_config import ModelConfig
    t = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    d = ModelConfig("llama", 128, 1, 2, 1, 64, 256, 512, 1e-5, 5e5, 1024, True)
    wt = W.synthetic_state_dict(t, seed=0, std=0.1)
    wd = W.synthetic_state_dict(d, seed=1, std=0.1)
    wd.pop("lm_head.weight", None)
    return t, d, wt, wd


def test_mixed_batch_base_and_two_adapters_with_prefix_cache_and_preemption(gpu):
    """max_num_seqs = 3: requests on the base, adapter X and adapter Y share steps, prompts share a 40-token prefix, and 16 blocks
    preempt.  Each stream against the oracle engine on its own weights (base, X-merged, Y-merged)."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.util import assert_stream_matches, seq_margins
    t, d, wt, wd = _small_models()
    X, Y = _adapter(t, 21), _adapter(t, 22)
    shared = [(7 * j + 3) % 512 for j in range(40)]
    prompts = [shared + [(11 * i + j) % 512 for j in range(5 + 3 * i)] for i in range(6)]
    names = [None, "x", "y", "x", None, "y"]
    kw = dict(hf_config=t, draft="d", draft_hf_config=d, speculate=True, speculate_k=3, max_num_seqs=3, max_model_len=256,
              max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=16, num_draft_kvcache_blocks=16)
    sp = lambda name: SamplingParams(temperature=0, max_new_tokens=14, ignore_eos=True, lora=name)
    eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), enable_lora=True, max_loras=4, max_lora_rank=16, **kw)
    eng.add_lora("x", X)
    eng.add_lora("y", Y)
    gpu_out, _ = eng.generate(prompts, [sp(n) for n in names], use_tqdm=False)
    assert any(k[0].endswith("_a") for k in eng.model_runner.graphs)
    eng.exit()
    weights_of = {None: wt, "x": LR.merge_state_dict(wt, X, t.num_layers)[0], "y": LR.merge_state_dict(wt, Y, t.num_layers)[0]}
    for name, wm in weights_of.items():
        idx = [i for i, n in enumerate(names) if n == name]
        cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(wm, wd), **kw)
        cpu_out, _ = cpu_eng.generate([prompts[i] for i in idx], sp(None), use_tqdm=False)
        for j, i in enumerate(idx):
            n = assert_stream_matches(gpu_out[i]["token_ids"], cpu_out[j]["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, j),
                                      len(prompts[i]), what=f"lora batch seq {i} on {name}")
            print(f"lora batch seq {i} on {name}: identical tokens {n} of {len(cpu_out[j]['token_ids'])}")
    streams = [tuple(o["token_ids"]) for o in gpu_out]
    assert len(set(streams)) > 3


def test_prefix_cache_roots_and_adapter_lifecycle(gpu):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    t, d, wt, wd = _small_models()
    kw = dict(hf_config=t, max_num_seqs=2, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=32)
    eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), enable_lora=True, max_loras=4, max_lora_rank=16, **kw)
    prompt = [(5 * j + 1) % 512 for j in range(40)]
    sp = lambda name, n=8: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True, lora=name)
    with pytest.raises(ValueError, match="lora='x'"):
        eng.add_request(prompt, sp("x"))
    X, Y, Z = _adapter(t, 31), _adapter(t, 32), _adapter(t, 33)
    eng.add_lora("x", X)
    hits = []
    real_allocate = eng.scheduler.block_manager.allocate

    def allocate(seq):
        real_allocate(seq)
        hits.append((seq.lora, seq.num_cached_tokens))
    eng.scheduler.block_manager.allocate = allocate
    out_x = eng.generate([prompt], sp("x"), use_tqdm=False)[0][0]["token_ids"]
    out_base = eng.generate([prompt], sp(None), use_tqdm=False)[0][0]["token_ids"]
    out_x2 = eng.generate([prompt], sp("x"), use_tqdm=False)[0][0]["token_ids"]
    assert hits == [("x", 0), (None, 0), ("x", 32)], hits      # base after X: no hit; X after X: the two full blocks
    assert out_x == out_x2 and out_x != out_base
    # replacing X by Z under the same name changes the stream and takes no stale prefix hit
    eng.remove_lora("x")
    assert eng.list_loras() == []
    eng.add_lora("x", Z)
    out_z = eng.generate([prompt], sp("x"), use_tqdm=False)[0][0]["token_ids"]
    assert hits[-1] == ("x", 0) and out_z != out_x
    # four slots: a fifth adapter is refused by name; an adapter in use cannot be removed
    eng.add_lora("y", Y)
    eng.add_lora("u", X)
    eng.add_lora("v", X)
    assert eng.list_loras() == ["x", "y", "u", "v"]
    with pytest.raises(ValueError, match="'w'.*max_loras"):
        eng.add_lora("w", Y)
    eng.add_request(prompt, sp("y"))
    with pytest.raises(ValueError, match="'y' is in use"):
        eng.remove_lora("y")
    eng.abort_all()
    eng.remove_lora("y")
    assert eng.list_loras() == ["x", "u", "v"]
    with pytest.raises(ValueError, match="r = 32 exceeds max_lora_rank = 16"):
        eng.add_lora("big", _adapter(t, 1, r=32))
    Sequence.block_size = 256
    eng.exit()


@pytest.mark.parametrize("mode", ["ar", "sync"])
def test_enable_lora_without_adapted_requests_launches_what_the_plain_engine_launches(gpu, monkeypatch, mode):
    """The ordered calls into ssd_amd.hip.ops / filter_ops / penalty_ops (recorded as tests/test_launch_trace_gpu.py records them)
    and the tokens of an engine with enable_lora=True -- one adapter registered, no request naming it -- equal the plain engine's;
    no adapter kernel is launched."""
    from ssd_amd.hip import lora_ops
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_launch_trace_gpu import install_recorder, make_engine, N_NEW
    runs = []
    for extra in ({}, dict(enable_lora=True, max_loras=2, max_lora_rank=16)):
        eng, prompts = make_engine(mode, extra, True)
        if extra:
            eng.add_lora("x", _adapter(eng.config.hf_config, 5))
        trace, lora_calls = [], []
        with monkeypatch.context() as mp:
            install_recorder(mp.setattr, trace)
            for name in ("lora_shrink", "lora_expand"):
                mp.setattr(lora_ops, name, lambda *a, _n=name, **k: lora_calls.append(_n))
            out, _ = eng.generate(prompts, SamplingParams(max_new_tokens=N_NEW, ignore_eos=True, temperature=0), use_tqdm=False)
        runs.append((trace, [o["token_ids"] for o in out], lora_calls))
        eng.exit()
    (t0, tok0, _), (t1, tok1, calls) = runs
    assert len(t0) > 20 and t0 == t1 and tok0 == tok1 and calls == []
