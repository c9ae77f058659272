"""A W8A16 (int8 weight-only, group 128) target end to end on the MI355X: model logits against float64 arithmetic on the exact weights
s * q (the bar of tests/test_w4a16_engine_gpu.py _logits_vs_truth: rms|HIP - f64| <= 1.25 rms|oracle - f64| + 1e-3 over all logits,
same argmax outside near-ties, the oracle being the unmodified CPU oracle given bf16(s * q) weights), a 300-row prompt through the
dequantize route, and a 24-token synchronous-speculation stream in lock step with the oracle engine on those weights."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def quantized(w: dict):
    """(bf16(s * q) weights for the oracle, f64 s * q weights for the truth): every decoder linear through the product quantizer."""
    from ssd_amd.quant import is_quantized_linear, quantize_w8a16, W8_GROUP
    bf, f64 = {}, {}
    for n, t in w.items():
        if is_quantized_linear(n):
            codes, s = quantize_w8a16(t.to("cuda"))
            exact = (codes.double() - 128) * s.double().repeat_interleave(W8_GROUP, dim=1)
            bf[n], f64[n] = exact.to(BF).cpu(), exact.cpu()
        else:
            bf[n], f64[n] = t, t
    return bf, f64


def _logits_vs_truth(cfg, w, prompt, n_verify, gpu, what):
    """HIP w8a16 decoder: prefill of the prompt, then one verify forward of n_verify rows; oracle (bf16(s*q) weights) and float64
    truth (exact s*q) over the whole sequence; the rows of both forwards are held to the rms bar."""
    from oracle.model import OracleModel, Ctx
    from ssd_amd.hip import ops as H
    from ssd_amd.model import HipDecoder, AttnMeta
    from tests.util import truth_forward
    wq, w64 = quantized(w)
    seq, P, T, bs = list(prompt), len(prompt) - n_verify, len(prompt), 16
    nblocks = -(-T // bs) + 1
    dec = HipDecoder(cfg, max_tokens=max(T, 64), max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=max(512, T + 16),
                     device=gpu, quantization="w8a16")
    drop = lambda d: {k: v for k, v in d.items() if not (cfg.tie_word_embeddings and k == "lm_head.weight")}
    dec.load_weights(iter(drop(w).items()))
    dec.alloc_kv(nblocks)
    slots = [p for p in range(T)]                       # block table 0, 1, 2, ...: slot = position
    bt = torch.tensor([list(range(nblocks))], dtype=torch.int32, device=gpu)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=gpu)
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device=gpu)
    dec.forward(i64(seq[:P]), i64(range(P)), P, AttnMeta(H.MODE_CAUSAL, 1, P, i32(slots[:P]), i32([P]), bt, cu_q=i32([0, P])))
    got_p = dec.logits[:dec.compute_logits(P)].double().cpu()
    dec.forward(i64(seq[P:]), i64(range(P, T)), n_verify, AttnMeta(H.MODE_CAUSAL, 1, n_verify, i32(slots[P:]), i32([T]), bt, q_per_seq=n_verify))
    got = torch.cat([got_p, dec.logits[:dec.compute_logits(n_verify)].double().cpu()])
    orc = OracleModel(cfg, drop(wq), nblocks, bs)
    cu = torch.tensor([0, T], dtype=torch.int32)
    ref_h = orc.forward(torch.tensor(seq), torch.arange(T), Ctx("prefill", slot_mapping=torch.tensor(slots, dtype=torch.int32), cu_q=cu, cu_k=cu))
    ref = orc.compute_logits(ref_h[0] if isinstance(ref_h, tuple) else ref_h).double()
    truth = truth_forward(cfg, drop(w64), seq)
    e_hip, e_ref = (got - truth).abs(), (ref - truth).abs()
    assert torch.isfinite(got).all()
    r_hip, r_ref = e_hip.pow(2).mean().sqrt().item(), e_ref.pow(2).mean().sqrt().item()
    print(f"{what}: rms |HIP - f64| {r_hip:.5f} max {e_hip.max():.4f} | rms |oracle - f64| {r_ref:.5f} max {e_ref.max():.4f}")
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: rms |HIP - f64| {r_hip:.5f} > 1.25 x {r_ref:.5f} + 1e-3"
    top2 = ref.topk(2, dim=-1).values
    thr = torch.clamp(2 * (got - ref).abs().max(-1).values, min=0.0625)
    assert bool(((got.argmax(-1) == ref.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all()), f"{what}: argmax differs beyond a near-tie"
    return dec


@pytest.mark.parametrize("name,family,kw", [("tiny_llama", "llama", {}), ("tiny_qwen3", "qwen3", dict(tie=True, qk_norm=True))])
def test_tiny_model_w8a16_logits(gpu, golden, name, family, kw):
    from tests.test_model_gpu import mk_cfg
    g = golden(name)
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    dec = _logits_vs_truth(mk_cfg(g, family, **kw), w, prompt, len(g["verify_tokens"]), gpu, f"{name} w8a16")
    assert dec.w8 and not (dec.fp8 or dec.w4 or dec.mx4) and dec.w["model.layers.0.mlp.down_proj.weight"].dtype == torch.uint8
    assert dec.w["model.layers.0.mlp.down_proj.weight_scale"].dtype == BF
    assert not (dec.chain_seg or dec.tree_seg or dec.use_parts or dec.pf_parts or dec.fuse_attn_o)


def test_300_row_prompt_takes_the_dequantize_route(gpu):
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    w = W.synthetic_state_dict(cfg, seed=7, std=0.05)
    random.seed(5)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(308)]
    assert 300 > HipDecoder.W8_DIRECT_MAX_T
    assert _logits_vs_truth(cfg, w, prompt, 8, gpu, "300-row prompt w8a16")._deq is not None


def test_w8a16_target_sync_speculation_lockstep_with_oracle(gpu, golden):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine, hip_runner_factory
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.utils.topology import Topology
    from tests.lockstep import compare_lockstep
    from tests.test_model_gpu import mk_cfg, weights
    g = golden("engine_golden")
    w = {False: weights(g, "t."), True: weights(g, "d.")}
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True, speculate_k=int(g["sd_K"]),
              max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)

    def factory(config, model_cfg, *, is_draft, topo, **k2):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(w[is_draft].items()), **k2)

    gpu_eng = LLMEngine("t", runner_factory=factory, quantization="w8a16", **kw)
    assert gpu_eng.model_runner.model.w8
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(quantized(w[False])[0], w[True]),
                        topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    rep = compare_lockstep(gpu_eng, cpu_eng, g["prompt"].tolist(), 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True), fan_out=None, what="w8a16 target sync")
    gpu_eng.exit()
    print(f"w8a16 target sync: {rep.summary()}")
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()
