"""An MXFP4 (e2m1 codes, e8m0 scale per 32 columns) target end to end on the MI355X: model logits against float64 arithmetic on the
exact dequantized weights (bar: rms|HIP - f64| <= 1.25 rms|oracle - f64| + 1e-3 and max|HIP - f64| <= 1.5 max|oracle - f64| + 1e-3 over
all logits, same argmax outside near-ties; the unmodified CPU oracle and the float64 truth get the SAME exact matrix, which is a bf16
matrix), prompts within the direct limit and at 300 rows (the dequantize route), greedy engine streams in lock step with the oracle
engine on those weights (sync and async speculation, batching + prefix caching), a pre-quantized checkpoint directory through
LLMEngine, the weight bytes of the 70B target, and a bf16 decoder beside it left as it was."""
import dataclasses
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
    """(the exact dequantized weights as bf16 for the oracle, the same as f64 for the truth): every decoder linear through the product
    quantizer (bit-exact against tests/mxfp4_ref.py in test_mxfp4_cpu.py) and the numpy restatement's exact product."""
    from ssd_amd.quant import is_quantized_linear, quantize_mxfp4
    from tests import mxfp4_ref as R
    bf, f64 = {}, {}
    for n, t in w.items():
        if is_quantized_linear(n):
            packed, s = quantize_mxfp4(t.to("cuda"))
            exact = torch.from_numpy(R.exact(R.unpack(packed.cpu().numpy()), s.cpu().numpy()))
            assert torch.equal(exact.to(BF).double(), exact)          # the dequantized matrix IS a bf16 matrix
            bf[n], f64[n] = exact.to(BF), exact
        else:
            bf[n], f64[n] = t, t
    return bf, f64


def _logits_vs_truth(cfg, w, prompt, n_verify, gpu, what):
    """HIP mxfp4 decoder: prefill of the prompt, then one verify forward of n_verify rows; oracle (exact dequantized weights) and float64
    truth (the same matrix) over the whole sequence; the rows of both forwards are held to the rms bar."""
    from oracle.model import OracleModel, Ctx
    from ssd_amd.hip import ops as H
    from ssd_amd.model import HipDecoder, AttnMeta
    from tests.util import truth_forward
    wq, w64 = quantized(w)
    seq = list(prompt)
    P, T = len(prompt) - n_verify, len(prompt)
    bs = 16
    nblocks = -(-T // bs) + 1
    dec = HipDecoder(cfg, max_tokens=max(T, 64), max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=max(512, T + 16),
                     device=gpu, quantization="mxfp4")
    ws = dict(w)
    if cfg.tie_word_embeddings:
        ws.pop("lm_head.weight", None)
    dec.load_weights(iter(ws.items()))
    dec.alloc_kv(nblocks)
    table = list(range(nblocks))
    bt = torch.tensor([table], dtype=torch.int32, device=gpu)
    sl = lambda ps: torch.tensor([table[p // bs] * bs + p % bs for p in ps], dtype=torch.int32, device=gpu)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=gpu)
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device=gpu)
    dec.forward(i64(seq[:P]), i64(range(P)), P, AttnMeta(H.MODE_CAUSAL, 1, P, sl(range(P)), i32([P]), bt, cu_q=i32([0, P])))
    n = dec.compute_logits(P)
    got_p = dec.logits[:n].double().cpu()
    dec.forward(i64(seq[P:]), i64(range(P, T)), n_verify,
                AttnMeta(H.MODE_CAUSAL, 1, n_verify, sl(range(P, T)), i32([T]), bt, q_per_seq=n_verify))
    n = dec.compute_logits(n_verify)
    got = torch.cat([got_p, dec.logits[:n].double().cpu()])
    drop = lambda d: {k: v for k, v in d.items() if not (cfg.tie_word_embeddings and k == "lm_head.weight")}
    orc = OracleModel(cfg, drop(wq), nblocks, bs)
    cu = torch.tensor([0, T], dtype=torch.int32)
    ref_h = orc.forward(torch.tensor(seq), torch.arange(T), Ctx("prefill", slot_mapping=torch.tensor([table[p // bs] * bs + p % bs for p in range(T)], dtype=torch.int32), cu_q=cu, cu_k=cu))
    ref_h = ref_h[0] if isinstance(ref_h, tuple) else ref_h
    ref = orc.compute_logits(ref_h).double()
    truth = truth_forward(cfg, drop(w64), seq)
    rms = lambda e: e.pow(2).mean(-1).sqrt()
    e_hip, e_ref = (got - truth).abs(), (ref - truth).abs()
    print(f"{what}: |HIP-f64| rms {rms(e_hip).mean():.5f} max {e_hip.max():.4f} | |oracle-f64| rms {rms(e_ref).mean():.5f} "
          f"max {e_ref.max():.4f}")
    assert torch.isfinite(got).all()
    r_hip, r_ref = e_hip.pow(2).mean().sqrt().item(), e_ref.pow(2).mean().sqrt().item()
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: rms |HIP - f64| {r_hip:.5f} > 1.25 x {r_ref:.5f} + 1e-3"
    assert e_hip.max().item() <= 1.5 * e_ref.max().item() + 1e-3, f"{what}: max |HIP - f64| {e_hip.max():.4f} > 1.5 x {e_ref.max():.4f} + 1e-3"
    top2 = ref.topk(2, dim=-1).values
    thr = torch.clamp(2 * (got - ref).abs().max(-1).values, min=0.0625)
    assert bool(((got.argmax(-1) == ref.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all()), f"{what}: argmax differs beyond a near-tie"
    return dec


def test_tiny_llama_mxfp4_logits(gpu, golden):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_llama")
    cfg = mk_cfg(g, "llama")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    dec = _logits_vs_truth(cfg, w, prompt, len(g["verify_tokens"]), gpu, "tiny llama mxfp4")
    assert dec.mx4 and not dec.fp8 and not dec.w4 and dec.w["model.layers.0.mlp.down_proj.weight"].dtype == torch.uint8
    assert dec.w["model.layers.0.mlp.down_proj.weight_scale"].dtype == torch.uint8
    assert not (dec.chain_seg or dec.tree_seg or dec.use_parts or dec.pf_parts or dec.fuse_attn_o)


def test_tiny_qwen3_mxfp4_logits(gpu, golden):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_qwen3")
    cfg = mk_cfg(g, "qwen3", tie=True, qk_norm=True)
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    _logits_vs_truth(cfg, w, prompt, len(g["verify_tokens"]), gpu, "tiny qwen3 mxfp4")


def test_300_row_prompt_takes_the_dequantize_route(gpu):
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    w = W.synthetic_state_dict(cfg, seed=7, std=0.05)
    random.seed(5)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(308)]
    assert 300 > HipDecoder.MX4_DIRECT_MAX_T
    dec = _logits_vs_truth(cfg, w, prompt, 8, gpu, "300-row prompt mxfp4")
    assert dec._deq is not None


def test_two_layer_70b_cut_mxfp4_logits(gpu):
    """A 160-token prompt (> the direct limit: dequantize + bf16 prefill) then an 8-row verify (the mxfp4 GEMM), 70B layer shapes."""
    from ssd_amd import weights as W
    from ssd_amd.model_config import PRESETS
    cfg = dataclasses.replace(PRESETS["llama-3.1-70b"], num_layers=2, vocab_size=16384)
    w = W.synthetic_state_dict(cfg, seed=4, std=0.02)
    random.seed(3)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(168)]
    _logits_vs_truth(cfg, w, prompt, 8, gpu, "70B x 2 layers mxfp4")


# ---------------------------------------------------------------------------------------------------------------------
# engine streams
# ---------------------------------------------------------------------------------------------------------------------
def _factory(w):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(w[is_draft].items()), **kw)
    return f


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_mxfp4_target_engine_lockstep_with_oracle(gpu, golden, mode):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.utils.topology import Topology
    from tests.lockstep import compare_lockstep
    from tests.test_model_gpu import mk_cfg, weights
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)
    if mode == "async":
        kw.update(speculate_k=3, draft_async=True, async_fan_out=2, jit_speculate=True)
    else:
        kw.update(speculate_k=int(g["sd_K"]))
    gpu_eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), inprocess_draft=mode == "async", quantization="mxfp4", **kw)
    assert gpu_eng.model_runner.model.mx4
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(quantized(wt)[0], wd), inprocess_draft=mode == "async",
                        topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    rep = compare_lockstep(gpu_eng, cpu_eng, g["prompt"].tolist(), 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True),
                           fan_out=2 if mode == "async" else None, what=f"mxfp4 target {mode}")
    gpu_eng.exit()
    print(f"mxfp4 target {mode}: {rep.summary()}")
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()


def test_mxfp4_target_batch_prefix_cache(gpu):
    """b > 1 with shared prefixes and preemption against the oracle engine on exact dequantized weights."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import ModelConfig
    from ssd_amd.sampling_params import SamplingParams
    from tests.util import assert_stream_matches, seq_margins
    t = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    d = ModelConfig("llama", 128, 1, 2, 1, 64, 256, 512, 1e-5, 5e5, 1024, True)
    wt = W.synthetic_state_dict(t, seed=0, std=0.1)
    wd = W.synthetic_state_dict(d, seed=1, std=0.1)
    wd.pop("lm_head.weight", None)
    shared = [(7 * j + 3) % 512 for j in range(40)]
    prompts = [shared + [(11 * i + j) % 512 for j in range(5 + 3 * i)] for i in range(4)]
    kw = dict(hf_config=t, draft="d", draft_hf_config=d, speculate=True, speculate_k=3, max_num_seqs=3, max_model_len=256,
              max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=16, num_draft_kvcache_blocks=16)
    sp = SamplingParams(temperature=0, max_new_tokens=14, ignore_eos=True)
    eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), quantization="mxfp4", **kw)
    gpu_out, _ = eng.generate(prompts, sp, use_tqdm=False)
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(quantized(wt)[0], wd), **kw)
    cpu_out, _ = cpu_eng.generate(prompts, sp, use_tqdm=False)
    for i, (a, b) in enumerate(zip(gpu_out, cpu_out)):
        n = assert_stream_matches(a["token_ids"], b["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, i), len(prompts[i]),
                                  what=f"mxfp4 batch/prefix seq {i}")
        print("mxfp4 batch/prefix: identical tokens", n, "of", len(b["token_ids"]))


def test_70b_mxfp4_weight_bytes_equal_the_formula_and_bf16_decoder_beside_it(gpu):
    """Every matrix of the full 80-layer 70B target (zero-valued: the byte count does not depend on the values): N K / 2 bytes of codes
    plus N K / 32 scale bytes per linear, plus the bf16 LM head and norms; a bf16 decoder built beside it holds no mx4 tensors."""
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import PRESETS
    from ssd_amd.quant import is_quantized_linear
    cfg = PRESETS["llama-3.1-70b"]
    shapes = W.param_shapes(cfg)
    lin = sum(torch.Size(s).numel() for n, s in shapes if is_quantized_linear(n))
    rest = sum(2 * torch.Size(s).numel() for n, s in shapes if not is_quantized_linear(n) and n != "model.embed_tokens.weight")
    want = lin // 2 + lin // 32 + rest
    dec = HipDecoder(cfg, max_tokens=16, max_seqs=1, max_blocks=2, block_size=256, max_model_len=512, device=gpu, quantization="mxfp4")
    dec.load_weights((n, torch.zeros(s, dtype=BF, device=gpu)) for n, s in shapes)
    got = dec.weight_bytes()
    print(f"70B weight bytes: mxfp4 {got / 1e9:.2f} GB (decoder linears {lin / 2e9:.2f} GB codes + {lin / 32e9:.2f} GB scales)")
    assert got == want
    assert abs(got / 1e9 - 38.47) < 0.01
    del dec
    torch.cuda.empty_cache()
    small = dataclasses.replace(cfg, num_layers=1, vocab_size=1024)
    sd = W.synthetic_state_dict(small, seed=2, std=0.02)
    kw = dict(max_tokens=16, max_seqs=1, max_blocks=2, block_size=256, max_model_len=512, device=gpu)
    q = HipDecoder(small, quantization="mxfp4", **kw)
    q.load_weights(iter(sd.items()))
    b = HipDecoder(small, **kw)
    b.load_weights(iter(sd.items()))
    assert not (b.mx4 or b.w4 or b.fp8 or b.quantized)
    assert not any(n.endswith("_scale") for n in b.w) and all(t.dtype != torch.uint8 for t in b.w.values())
    assert sorted(n for n in q.w if not n.endswith("_scale")) == sorted(b.w)
    assert b.w["model.layers.0.mlp.down_proj.weight"].dtype == BF and q.w["model.layers.0.mlp.down_proj.weight"].dtype == torch.uint8


def test_llm_engine_generates_from_a_prequantized_mxfp4_checkpoint_directory(gpu, tmp_path):
    """LLMEngine(<directory>, quantization="mxfp4") on a synthetic mxfp4-pack-quantized checkpoint: codes and scales reach the decoder
    bit for bit (read back through ssd_mx4_frag_to_rows), and the greedy stream equals the one of the same engine fed the exact
    dequantized bf16 weights with quantize-on-load (quantizing an exact MXFP4 matrix reproduces its values)."""
    import json
    import os
    from safetensors.torch import save_file
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.hip import mx4_ops as MX4
    from ssd_amd.model_config import ModelConfig
    from ssd_amd.quant import is_quantized_linear, quantize_mxfp4, dequantize_mxfp4, gate_up_row_map
    from ssd_amd.sampling_params import SamplingParams
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    sd = W.synthetic_state_dict(cfg, seed=3, std=0.05)
    hf_names = {"self_attn.qkv_proj": (("self_attn.q_proj", 256), ("self_attn.k_proj", 128), ("self_attn.v_proj", 128)),
                "mlp.gate_up_proj": (("mlp.gate_proj", 512), ("mlp.up_proj", 512))}
    tensors, deq, kept = {}, {}, {}
    for n, t in sd.items():
        if is_quantized_linear(n):
            q = quantize_mxfp4(t)
            deq[n], kept[n] = dequantize_mxfp4(*q), q
            base = n[:-len(".weight")]
            key = next((k for k in hf_names if base.endswith(k)), None)
            if key is None:
                tensors[base + ".weight_packed"], tensors[base + ".weight_scale"] = q.packed, q.scale
            else:                      # unpacked q / k / v and gate / up, as a Hugging Face checkpoint stores them
                r0, prefix = 0, base[:-len(key)]
                for part, rows in hf_names[key]:
                    tensors[prefix + part + ".weight_packed"] = q.packed[r0:r0 + rows].contiguous()
                    tensors[prefix + part + ".weight_scale"] = q.scale[r0:r0 + rows].contiguous()
                    r0 += rows
        else:
            tensors[n], deq[n] = t.contiguous(), t
    d = str(tmp_path)
    save_file(tensors, os.path.join(d, "model.safetensors"))
    wq = {"num_bits": 4, "type": "float", "symmetric": True, "strategy": "group", "group_size": 32, "dynamic": False}
    qc = {"quant_method": "compressed-tensors", "format": "mxfp4-pack-quantized", "ignore": ["lm_head"],
          "config_groups": {"group_0": {"targets": ["Linear"], "weights": wq, "input_activations": None}}}
    hf = {"model_type": "llama", "architectures": ["LlamaForCausalLM"], "hidden_size": 256, "num_hidden_layers": 2,
          "num_attention_heads": 4, "num_key_value_heads": 2, "head_dim": 64, "intermediate_size": 512, "vocab_size": 512,
          "rms_norm_eps": 1e-5, "rope_theta": 5e5, "max_position_embeddings": 1024, "tie_word_embeddings": False,
          "quantization_config": qc}
    json.dump(hf, open(os.path.join(d, "config.json"), "w"))
    assert W.checkpoint_quantization(d) == "mxfp4"
    kw = dict(hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=32)
    sp = SamplingParams(temperature=0, max_new_tokens=12, ignore_eos=True)
    prompt = [(5 * j + 1) % 512 for j in range(20)]
    eng = LLMEngine(d, quantization="mxfp4", **kw)
    dec = eng.model_runner.model
    assert dec.mx4
    n = "model.layers.1.mlp.gate_up_proj.weight"
    N, K = 2 * cfg.intermediate_size, cfg.hidden_size
    bq = torch.empty(N, K // 2, dtype=torch.uint8, device=gpu)
    bs = torch.empty(N, K // 32, dtype=torch.uint8, device=gpu)
    MX4.mx4_frag_to_rows(dec.w[n], dec.w[n + "_scale"], bq, bs, N, K)
    order = gate_up_row_map(N).long()
    assert torch.equal(bq.cpu(), kept[n].packed[order]) and torch.equal(bs.cpu(), kept[n].scale[order])
    out_ckpt, _ = eng.generate([prompt], sp, use_tqdm=False)
    eng.exit()
    eng2 = LLMEngine("t", runner_factory=_factory({False: deq, True: deq}), quantization="mxfp4", **kw)
    out_deq, _ = eng2.generate([prompt], sp, use_tqdm=False)
    eng2.exit()
    assert len(out_ckpt[0]["token_ids"]) == 12 and out_ckpt[0]["token_ids"] == out_deq[0]["token_ids"]
