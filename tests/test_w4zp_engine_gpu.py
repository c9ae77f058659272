"""A W4A16 target with zero points end to end on the MI355X, in the pattern of tests/test_w4a16_engine_gpu.py: model logits against
float64 arithmetic on the exact weights s * (u - z) (bar: rms|HIP - f64| <= 1.25 rms|oracle - f64| + 1e-3 and max <= 1.5 max + 1e-3
over all logits, same argmax outside near-ties, the oracle being the unmodified CPU oracle given bf16(s * (u - z)) weights), prompts
within the direct limit and at 300 rows (the dequantize route), greedy engine streams in lock step with the oracle engine on those
weights (sync and async speculation, hipGraphs), tiny AutoAWQ and GPTQ checkpoint directories through LLM(dir, quantization="w4a16"),
symmetric and zero-point linears mixed in one model, and the weight bytes of the 70B target."""
import dataclasses
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import w4zp_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def quantized(w: dict):
    """(bf16(s * (u - z)) weights for the oracle, f64 s * (u - z) weights for the truth): every decoder linear through the product
    quantizer (bit-exact against tests/w4zp_ref.py in test_w4zp_cpu.py)."""
    from ssd_amd.quant import is_quantized_linear, quantize_w4a16_zp, unpack_w4u, dequantize_w4zp, W4_GROUP
    bf, f64 = {}, {}
    for n, t in w.items():
        if is_quantized_linear(n):
            q = quantize_w4a16_zp(t.to("cuda"))
            exact = (unpack_w4u(q.packed).double() - q.zero.double().repeat_interleave(W4_GROUP, dim=1)) \
                * q.scale.double().repeat_interleave(W4_GROUP, dim=1)
            bf[n], f64[n] = dequantize_w4zp(*q).cpu(), exact.cpu()
        else:
            bf[n], f64[n] = t, t
    return bf, f64


def _logits_vs_truth(cfg, w, prompt, n_verify, gpu, what):
    """HIP w4a16 decoder with the zero-point on-load quantizer: prefill of the prompt, then one verify forward of n_verify rows;
    oracle (bf16(s (u - z)) weights) and float64 truth (exact s (u - z)) over the whole sequence; the rows of both forwards are held
    to the rms and max bars."""
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
                     device=gpu, quantization="w4a16", w4_zero_point=True)
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
    m_hip, m_ref = e_hip.max().item(), e_ref.max().item()
    assert m_hip <= 1.5 * m_ref + 1e-3, f"{what}: max |HIP - f64| {m_hip:.5f} > 1.5 x {m_ref:.5f} + 1e-3"
    top2 = ref.topk(2, dim=-1).values
    thr = torch.clamp(2 * (got - ref).abs().max(-1).values, min=0.0625)
    assert bool(((got.argmax(-1) == ref.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all()), f"{what}: argmax differs beyond a near-tie"
    return dec


def test_tiny_llama_w4zp_logits(gpu, golden):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_llama")
    cfg = mk_cfg(g, "llama")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    dec = _logits_vs_truth(cfg, w, prompt, len(g["verify_tokens"]), gpu, "tiny llama w4a16 zero-point")
    n = "model.layers.0.mlp.down_proj.weight"
    assert dec.w4 and dec.w4_zero_point and dec.w[n].dtype == torch.uint8 and dec.w[n + "_scale"].dtype == BF
    assert dec.w[n + "_zero"].dtype == torch.uint8 and dec.w[n + "_zero"].numel() == dec.w[n + "_scale"].numel()
    assert not (dec.chain_seg or dec.tree_seg or dec.use_parts or dec.pf_parts or dec.fuse_attn_o)


def test_tiny_qwen3_w4zp_logits(gpu, golden):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_qwen3")
    cfg = mk_cfg(g, "qwen3", tie=True, qk_norm=True)
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    _logits_vs_truth(cfg, w, prompt, len(g["verify_tokens"]), gpu, "tiny qwen3 w4a16 zero-point")


def test_300_row_prompt_takes_the_dequantize_route(gpu):
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    w = W.synthetic_state_dict(cfg, seed=7, std=0.05)
    random.seed(5)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(308)]
    assert 300 > HipDecoder.W4_DIRECT_MAX_T
    dec = _logits_vs_truth(cfg, w, prompt, 8, gpu, "300-row prompt w4a16 zero-point")
    assert dec._deq is not None


def test_two_layer_70b_cut_w4zp_logits(gpu):
    """A 160-token prompt (> the direct limit: dequantize + bf16 prefill) then an 8-row verify (the zero-point GEMM), 70B layer shapes."""
    from ssd_amd import weights as W
    from ssd_amd.model_config import PRESETS
    cfg = dataclasses.replace(PRESETS["llama-3.1-70b"], num_layers=2, vocab_size=16384)
    w = W.synthetic_state_dict(cfg, seed=4, std=0.02)
    random.seed(3)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(168)]
    _logits_vs_truth(cfg, w, prompt, 8, gpu, "70B x 2 layers w4a16 zero-point")


# ---------------------------------------------------------------------------------------------------------------------
# engine streams
# ---------------------------------------------------------------------------------------------------------------------
def _factory(w):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(w[is_draft].items()), **kw)
    return f


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_w4zp_target_engine_lockstep_with_oracle(gpu, golden, mode):
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
    gpu_eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), inprocess_draft=mode == "async", quantization="w4a16",
                        w4_zero_point=True, **kw)
    dec = gpu_eng.model_runner.model
    assert dec.w4 and dec.w4_zero_point and "model.layers.0.self_attn.qkv_proj.weight_zero" in dec.w
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(quantized(wt)[0], wd), inprocess_draft=mode == "async",
                        topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    rep = compare_lockstep(gpu_eng, cpu_eng, g["prompt"].tolist(), 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True),
                           fan_out=2 if mode == "async" else None, what=f"w4a16 zero-point target {mode}")
    gpu_eng.exit()
    print(f"w4a16 zero-point target {mode}: {rep.summary()}")
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()


HF_PARTS = {"self_attn.qkv_proj": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"),
            "mlp.gate_up_proj": ("mlp.gate_proj", "mlp.up_proj")}


def _write_checkpoint(d, cfg, sd, kind, symmetric_names=()):
    """sd's decoder linears through the zero-point quantizer (the symmetric one for `symmetric_names`), written as an AutoAWQ
    ("awq") or GPTQ ("gptq": format gptq, stored zero = z - 1) checkpoint with unpacked q / k / v and gate / up, fp16 scales, norms,
    embedding and LM head.  Returns {packed name: W4ZTensor on the CPU} as quantized."""
    from safetensors.torch import save_file
    from ssd_amd.quant import is_quantized_linear, quantize_w4a16_zp, quantize_w4a16, unpack_w4u, W4ZTensor
    hd, nh, nkv, I = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size
    rows = {"self_attn.qkv_proj": (nh * hd, nkv * hd, nkv * hd), "mlp.gate_up_proj": (I, I)}
    tensors, kept = {}, {}
    for n, t in sd.items():
        if not is_quantized_linear(n):
            tensors[n] = t.to(torch.float16).contiguous()
            continue
        if n.endswith(tuple(s + ".weight" for s in symmetric_names)):
            q4 = quantize_w4a16(t)
            q = W4ZTensor(q4.packed, q4.scale, torch.full(q4.scale.shape, 8, dtype=torch.uint8))
        else:
            q = quantize_w4a16_zp(t)
        kept[n] = q
        u, s, z = unpack_w4u(q.packed).numpy(), q.scale.to(torch.float16), q.zero.numpy()
        assert torch.equal(s.to(BF), q.scale), "a bf16 scale of this size is exact in fp16"
        base = n[:-len(".weight")]
        key = next((k for k in HF_PARTS if base.endswith(k)), None)
        parts = [(base, 0, u.shape[0])] if key is None else []
        r0 = 0
        for part, nr in zip(HF_PARTS.get(key, ()), rows.get(key, ())):
            parts.append((base[:-len(key)] + part, r0, r0 + nr))
            r0 += nr
        for name, a, b in parts:
            pk = R.awq_pack(u[a:b], s.numpy()[a:b], z[a:b]) if kind == "awq" else R.gptq_pack(u[a:b], s.numpy()[a:b], z[a:b], v1=True)
            for suffix, arr in pk.items():
                tensors[name + "." + suffix] = torch.from_numpy(np.ascontiguousarray(arr))
    save_file(tensors, os.path.join(d, "model.safetensors"))
    if kind == "awq":
        qc = {"quant_method": "awq", "bits": 4, "group_size": 128, "zero_point": True, "version": "gemm", "modules_to_not_convert": None}
    else:
        qc = {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False, "sym": False, "checkpoint_format": "gptq"}
    hf = {"model_type": "llama", "architectures": ["LlamaForCausalLM"], "hidden_size": cfg.hidden_size,
          "num_hidden_layers": cfg.num_layers, "num_attention_heads": nh, "num_key_value_heads": nkv, "head_dim": hd,
          "intermediate_size": I, "vocab_size": cfg.vocab_size, "rms_norm_eps": 1e-5, "rope_theta": 5e5,
          "max_position_embeddings": 1024, "tie_word_embeddings": False, "quantization_config": qc}
    json.dump(hf, open(os.path.join(d, "config.json"), "w"))
    return kept


@pytest.mark.parametrize("kind", ["awq", "gptq"])
def test_llm_generates_from_an_int4_checkpoint_directory(gpu, tmp_path, kind):
    """LLM(<directory>, quantization="w4a16") on a tiny AutoAWQ / GPTQ checkpoint: codes, scales and zero points reach the decoder bit
    for bit (read back through ssd_w4zp_frag_to_rows, in the packed row orders), a linear whose zero points are all 8 lands on the
    symmetric kernel (no zero table), and the greedy stream equals the oracle engine's on bf16(s (u - z)) weights."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd import weights as W
    from ssd_amd.llm import LLM
    from ssd_amd.hip import w4zp_ops as W4Z
    from ssd_amd.model_config import ModelConfig
    from ssd_amd.quant import dequantize_w4zp, gate_up_row_map, qkv_row_map
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.util import assert_stream_matches, seq_margins
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    sd = W.synthetic_state_dict(cfg, seed=3, std=0.05)
    sd = {n: (t.to(torch.float16).to(BF) if t.dim() < 2 or not n.startswith("model.layers.") else t) for n, t in sd.items()}
    d = str(tmp_path)
    kept = _write_checkpoint(d, cfg, sd, kind, symmetric_names=("self_attn.o_proj",))
    assert W.checkpoint_quantization(d) == "w4a16"
    kw = dict(hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=32)
    sp = SamplingParams(temperature=0, max_new_tokens=12, ignore_eos=True)
    prompt = [(5 * j + 1) % 512 for j in range(20)]
    eng = LLM(d, quantization="w4a16", **kw)
    dec = eng.model_runner.model
    assert dec.w4 and not dec.w4_zero_point
    for n, order in (("model.layers.1.mlp.gate_up_proj.weight", gate_up_row_map(2 * cfg.intermediate_size).long()),
                     ("model.layers.0.self_attn.qkv_proj.weight", qkv_row_map(4, 2, 64).long()),
                     ("model.layers.1.mlp.down_proj.weight", None)):
        N, K = kept[n].packed.shape[0], kept[n].packed.shape[1] * 8
        bq = torch.empty(N, K // 8, dtype=torch.int32, device=gpu)
        bs = torch.empty(N, K // 128, dtype=BF, device=gpu)
        bz = torch.empty(N, K // 128, dtype=torch.uint8, device=gpu)
        W4Z.w4zp_frag_to_rows(dec.w[n], dec.w[n + "_scale"], dec.w[n + "_zero"], bq, bs, bz, N, K)
        order = torch.arange(N) if order is None else order
        assert torch.equal(bq.cpu(), kept[n].packed[order]) and torch.equal(bz.cpu(), kept[n].zero[order]), n
        assert torch.equal(bs.cpu().view(torch.int16), kept[n].scale[order].view(torch.int16)), n
    assert "model.layers.0.self_attn.o_proj.weight_zero" not in dec.w and "model.layers.0.self_attn.o_proj.weight_scale" in dec.w
    out, _ = eng.generate([prompt], sp, use_tqdm=False)
    eng.exit()
    wq = {n: (dequantize_w4zp(*kept[n]) if n in kept else t.to(torch.float16).to(BF)) for n, t in sd.items()}
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(wq, None), **kw)
    ref, _ = cpu_eng.generate([prompt], sp, use_tqdm=False)
    n = assert_stream_matches(out[0]["token_ids"], ref[0]["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, 0), len(prompt),
                              what=f"{kind} checkpoint directory")
    print(f"{kind} checkpoint directory: identical tokens {n} of {len(ref[0]['token_ids'])}")
    assert len(out[0]["token_ids"]) == 12


def test_70b_w4zp_weight_bytes_equal_the_formula(gpu):
    """Every matrix of the full 80-layer 70B target (zero-valued: the byte count does not depend on the values): codes at half a byte
    per weight, one bf16 scale and one zero-point byte per 128 weights -- 1072 bytes per unit against the symmetric 1056."""
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import PRESETS
    from ssd_amd.quant import is_quantized_linear
    cfg = PRESETS["llama-3.1-70b"]
    shapes = W.param_shapes(cfg)
    lin = sum(torch.Size(s).numel() for n, s in shapes if is_quantized_linear(n))
    rest = sum(2 * torch.Size(s).numel() for n, s in shapes if not is_quantized_linear(n) and n != "model.embed_tokens.weight")
    want = lin // 2 + 3 * (lin // 128) + rest
    dec = HipDecoder(cfg, max_tokens=16, max_seqs=1, max_blocks=2, block_size=256, max_model_len=512, device=gpu, quantization="w4a16",
                     w4_zero_point=True)
    dec.load_weights((n, torch.zeros(s, dtype=BF, device=gpu)) for n, s in shapes)
    got = dec.weight_bytes()
    print(f"70B weight bytes: w4a16 zero-point {got / 1e9:.2f} GB")
    assert got == want
