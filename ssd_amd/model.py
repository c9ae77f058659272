"""The decoder forward on MI355X: a fixed sequence of libssdhip launches over pre-allocated buffers.

Functionally LlamaForCausalLM.forward / Qwen3ForCausalLM.forward + compute_logits of the reference
(ssd/models/llama3.py:89-99,185-199,248-273; ssd/models/qwen3.py:90-108; ssd/layers/embed_head.py:78-116), with
the process-global attention Context (ssd/utils/context.py) turned into explicit arguments.

Per layer the launch list is: add+RMSNorm -> QKV GEMM -> (head-norm)+RoPE+KV-store -> paged attention
(+split merge) -> O GEMM [+all-reduce] -> add+RMSNorm -> gate_up GEMM with fused SiLU*mul -> down GEMM
[+all-reduce].  Activations that feed a GEMM are produced directly in the fragment-major layout; nothing is
allocated during a forward, so the whole thing can be captured in a hipGraph (torch.cuda.CUDAGraph is
hipGraph on ROCm) including the RCCL all-reduces.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import os

import torch
import torch.distributed as dist

from ssd_amd.hip import ops as H
from ssd_amd.hip import quant_ops as Q
from ssd_amd.hip import fp8b_ops as F8B
from ssd_amd.hip import w4_ops as W4
from ssd_amd.hip import w4zp_ops as W4Z
from ssd_amd.hip import mx4_ops as MX4
from ssd_amd.hip import kv8_ops as KV8
from ssd_amd.hip import lora_ops as LO
from ssd_amd.hip import moe_ops as MOE
from ssd_amd import lora as LR
from ssd_amd import quant
from ssd_amd.model_config import ModelConfig

BF16 = torch.bfloat16


@dataclass
class AttnMeta:
    """What the reference keeps in its global Context, plus the tree geometry."""
    mode: int                     # H.MODE_CAUSAL | H.MODE_TREE
    B: int
    max_q: int
    slot_mapping: torch.Tensor    # int32 [T]
    context_lens: torch.Tensor    # int32 [B]
    block_tables: torch.Tensor    # int32 [B, max_blocks]
    cu_q: torch.Tensor | None = None
    q_per_seq: int = 0
    tree_K: int = 0
    tree_mq: int = 0
    tree_step: int = 0
    tree_F: int = 1
    tree_jidx: torch.Tensor | None = None
    ctx_hint: int = 0             # host-side upper bound of the context lengths (0 = unknown -> max_model_len)


class Slabs(NamedTuple):
    """Where a GEMM left its result when not as bf16 rows in buf_h (that hand-off is None): fp32 split-K slabs [n][rows][h], summed by
    the consumer's norm -- buf_parts_o / buf_parts_d (ssd_gemm_parts, attention + o_proj) or the prefill workspace (PF_EPI_PARTIALS)."""
    buf: torch.Tensor
    n: int
    rows: int


NORMED = "normed"       # hand-off marker: the fused all-reduce + add + RMSNorm already left buf_xf / buf_res as the consumer's norm would
_PLAN = "plan"          # default of launch_*(src=): the hand-off parts_plan(T) implies (the launches taken one by one: bench.py, probes)


def make_cos_sin(head_dim: int, max_pos: int, theta: float, device) -> torch.Tensor:
    """fp32 [max_pos, hd] = cos || sin, computed on the host exactly as RotaryEmbedding.__init__ does
    (ssd/layers/rotary_embedding.py:28-36) -- never sinf/cosf on the device."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float) / head_dim))
    t = torch.arange(max_pos, dtype=torch.float)
    freqs = torch.einsum("i,j -> ij", t, inv_freq)
    return torch.cat((freqs.cos(), freqs.sin()), dim=-1).contiguous().to(device)


class HipDecoder:
    def __init__(self, cfg: ModelConfig, *, max_tokens: int, max_seqs: int, max_blocks: int, block_size: int,
                 max_model_len: int, device: torch.device, tp_rank: int = 0, tp_size: int = 1, tp_group=None,
                 max_logit_rows: int | None = None, max_split_tokens: int = 256, force_collectives: bool = False,
                 taps: list[int] | None = None, quantization: str | None = None, w4_zero_point: bool = False,
                 kv_cache_dtype: str | None = None, max_loras: int = 0, max_lora_rank: int = 64):
        self.cfg, self.device = cfg, device
        # cfg.num_experts > 0 (Qwen3-MoE): the MLP of every layer is a router + routed experts (include/ssd_hip_moe.h).  The decoder
        # takes the ROWS route exactly as a quantized target does -- every fused form off -- and launch_gate_up / launch_down, the only
        # two places the MLP lives, run add + norm (rows and frag), router GEMM, route, grouped up GEMM | grouped down GEMM, combine.
        # bf16 tables, bf16 KV, one rank, no adapters, no taps (Config refuses the rest by name).
        self.moe = cfg.num_experts > 0
        self.moe_trace: list | None = None      # debug hook: a list -> every eager MoE layer appends (router_logits.cpu(), topk_ids.cpu())
        assert not self.moe or (tp_size == 1 and not force_collectives and taps is None and quantization is None
                                and kv_cache_dtype is None and max_loras == 0), "MoE targets are single-rank bf16, without taps or adapters"
        # max_loras > 0 (Config.enable_lora): slot tables of LoRA adapters for the four linears of every layer (include/ssd_hip_lora.h,
        # ssd_amd/lora.py), allocated once at the end of __init__ -- before the KV cache is sized, so their memory is counted.  A
        # forward whose batch has an adapted row (lora_active, set by the runner with the row_slot array) takes the ROWS route of
        # every linear, as the quantized targets do, and adds the delta to those rows; a forward without one is launch for launch the
        # forward of a decoder without tables.  Single rank, no taps.
        assert max_loras == 0 or (tp_size == 1 and not force_collectives and taps is None), "LoRA targets are single-rank, without taps"
        assert max_loras == 0 or (1 <= max_loras <= LR.MAX_LORAS and max_lora_rank in LR.RANKS), (max_loras, max_lora_rank)
        self.max_loras, self.max_lora_rank = max_loras, max_lora_rank
        self.lora_active = False
        # kv_cache_dtype="fp8": the paged KV cache holds e4m3 codes, one byte per element, with one fp32 scale per layer, K or V, and kv
        # head (include/ssd_hip_kv8.h; all 1.0 until set_kv_scales).  Orthogonal to `quantization`.  Every form that writes or reads KV
        # inside another kernel is off -- the QKV + RoPE epilogue of gemm_fused (and with it the fused norm prologues, whose residual
        # ping-pong starts in that launch), attention + o_proj, the chain / tree segments, the QKV prefill partials -- so a layer is
        # QKV rows -> ssd_rope_store_kv_fp8 -> ssd_attn_paged_fp8; o / down partial slabs and the prefill forms stay as they are.
        if kv_cache_dtype not in (None, "fp8"):
            raise ValueError(f"kv_cache_dtype must be None or 'fp8', got {kv_cache_dtype!r}")
        self.kv8 = kv_cache_dtype == "fp8"
        if self.kv8 and cfg.head_dim not in (64, 128):
            raise ValueError(f"kv_cache_dtype='fp8' needs head_dim 64 or 128, got {cfg.head_dim}")
        assert not self.kv8 or (tp_size == 1 and not force_collectives and taps is None), "fp8 KV caches are single-rank, without taps"
        # quantization="fp8" | "w4a16" | "mxfp4": the decoder linears are codes + side tables in the format's device form (the formats
        # and their host forms: ssd_amd/quant.py; load_weights) and run on that format's GEMM (_gemm).  Every bf16-only fused form
        # (norm prologues, the QKV+RoPE epilogue, split-K slabs, attention + o_proj, the resident chain / tree segments, prefill
        # partials) is off, so a layer is norm -> GEMM -> RoPE / KV store -> attention -> GEMM -> norm -> GEMM -> GEMM.  Which GEMM a
        # linear runs on follows from the tables it has, so per-row and block-scaled fp8 linears, and symmetric and zero-point int4
        # ones (w4_zero_point=True: the on-load quantizer makes the latter), mix freely in one model.  Single rank only (Config
        # refuses the rest).
        assert quantization in (None, "fp8", "w4a16", "mxfp4"), quantization
        self.fp8 = quantization == "fp8"
        self.w4 = quantization == "w4a16"
        self.mx4 = quantization == "mxfp4"
        self.quantized = self.fp8 or self.w4 or self.mx4
        if w4_zero_point and not self.w4:
            raise ValueError(f"w4_zero_point=True needs quantization='w4a16', got {quantization!r}")
        self.w4_zero_point = w4_zero_point
        assert not self.quantized or (tp_size == 1 and not force_collectives and taps is None), \
            f"{quantization} targets are single-rank, without taps"
        self.tp_rank, self.tp_size, self.tp_group = tp_rank, tp_size, tp_group
        # force_collectives: issue the RCCL calls even at tp_size == 1 (lets a single-GPU box exercise the
        # collective + hipGraph-capture path that the multi-GPU runs depend on)
        self.use_coll = tp_size > 1 or (force_collectives and tp_group is not None)
        self.custom_ar = None      # OneShotAllReduce (ssd_amd/utils/custom_ar.py) once the runner has validated it
        self.fuse_ar_norm = True            # (all-reduce + add + RMSNorm in one launch; a probe may clear the attribute for an A/B run)
        assert cfg.num_heads % tp_size == 0 and cfg.num_kv_heads % tp_size == 0
        assert cfg.intermediate_size % (tp_size * 32) == 0 and cfg.vocab_size % (tp_size * 16) == 0
        self.nh, self.nkv = cfg.num_heads // tp_size, cfg.num_kv_heads // tp_size
        self.hd, self.h = cfg.head_dim, cfg.hidden_size
        self.I = cfg.moe_intermediate_size if self.moe else cfg.intermediate_size // tp_size
        self.V = cfg.vocab_size // tp_size
        self.qkv_n = (self.nh + 2 * self.nkv) * self.hd
        self.qn = self.nh * self.hd
        if self.w4 and any(k % quant.W4_GROUP for k in (self.h, self.qn, self.I)):
            raise ValueError(f"quantization='w4a16' needs hidden_size, num_heads * head_dim and intermediate_size to be multiples of "
                             f"{quant.W4_GROUP} (the group size), got {self.h}, {self.qn}, {self.I}")
        if self.mx4 and any(k % quant.MX4_GROUP for k in (self.h, self.qn, self.I)):
            raise ValueError(f"quantization='mxfp4' needs hidden_size, num_heads * head_dim and intermediate_size to be multiples of "
                             f"{quant.MX4_GROUP} (four 32-column blocks: one device unit), got {self.h}, {self.qn}, {self.I}")
        self.block_size, self.max_blocks = block_size, max_blocks
        self.max_tokens = max_tokens
        self.max_logit_rows = max_logit_rows or max_tokens
        self.max_split_tokens = max_split_tokens
        self.max_model_len = max_model_len
        self.w: dict[str, torch.Tensor] = {}
        self.kv_cache: torch.Tensor | None = None
        self.cos_sin = make_cos_sin(self.hd, max_model_len, cfg.rope_theta, device)

        def z(*shape, dtype=BF16):
            return torch.zeros(*shape, dtype=dtype, device=device)

        T = max_tokens
        self.buf_h = z(T, self.h)
        self.buf_res = z(T, self.h)
        self.buf_res2 = z(min(T, 16), self.h)      # second residual buffer of the fused decode path (ping-pong)
        self.buf_xf = z(H.frag_numel(T, self.h))
        self.buf_qkv = z(T, self.qkv_n)
        self.buf_q = z(T, self.qn)
        self.buf_af = z(H.frag_numel(T, self.qn))
        self.buf_actf = z(H.frag_numel(T, self.I))
        self.buf_lastf = z(H.frag_numel(self.max_logit_rows, self.h))
        # split-K partial slabs of o_proj / down_proj for models whose hidden size gives too few 16-row groups to fill
        # the chip (csrc/gemm_sk.hip gemm_sp_kernel): fp32 [S][T][h], summed by the consumer's prologue / ssd_rmsnorm_parts
        # (< 256 row groups: the 1B / 0.6B drafts; 256 < groups < 512: a quarter-empty second round of workgroups --
        # Qwen3-32B o_proj 20.6 -> 15.6 us, down_proj 58.1 -> 48.1 us at 16 splits, profiles/r02_parts_probe.txt; at exactly
        # 256 or >= 512 groups the rows kernels are as fast or faster)
        g_ = self.h // 16
        self.use_parts = g_ < 256 or 256 < g_ < 512
        # ssd_gemm_parts keeps a wave's whole K share in registers: <= 8 k-tiles per wave.  A shape whose (splits, waves) plan
        # cannot meet that (e.g. h = 3072 with I = 14336 under the two-slab fused consumer) runs the rows kernels instead
        def fits(N, K, fused):
            S, wv = self._parts_cfg(N, K, fused)
            return -(-(-(-(K // 32) // S)) // wv) <= 8
        fused_possible = (not cfg.qk_norm) and self.h // 8 <= 1024          # fusion_plan(): the norm prologue exists at T = 1 only
        if self.use_parts and not all(fits(self.h, k, f) for k in (self.qn, self.I) for f in ((False, True) if fused_possible else (False,))):
            self.use_parts = False
        self.fuse_attn_o = True
        self.pf_parts = True
        if self.quantized or self.moe:
            self.use_parts = self.fuse_attn_o = self.pf_parts = False
        if self.kv8:
            self.fuse_attn_o = False
        # fp8 KV: scale and inverse-scale tables fp32 [L][2 (K | V)][nkv], allocated once (hipGraphs bake the pointers)
        self.kv_scale = torch.ones(cfg.num_layers, 2, self.nkv, dtype=torch.float32, device=device) if self.kv8 else None
        self.kv_inv_scale = torch.ones_like(self.kv_scale) if self.kv8 else None
        # the single-token chain (one sequence, T = 1) with everything between two attention launches in ONE resident launch
        # (csrc/chain.hip): 1 + 2 per layer launches instead of 4 per layer
        # Default ("auto"): on at the geometry it was validated and measured at on the MI355X -- Llama-3.2-1B's, the draft of every
        # Llama configuration in BASELINE.json (tests/test_hip_chain.py, the full-size lock-step tests; draft forward 0.740 ->
        # 0.705 ms, c2 7.78 -> 7.50 ms / step, profiles/r04_chain_segment.txt).  SSD_CHAIN_SEG=1 forces it for every shape the
        # kernel accepts, =0 turns it off.
        _cs = os.environ.get("SSD_CHAIN_SEG", "auto")
        _geo = (self.h, self.qn, self.I, self.qkv_n, self.hd)
        _validated = _geo == (2048, 2048, 8192, 3072, 64)
        self.chain_seg = ((_cs == "1" or (_cs == "auto" and _validated)) and not cfg.qk_norm and tp_size == 1 and not self.use_coll and not self.quantized
                          and not self.moe and not self.kv8 and taps is None and H.chain_segment_ok(self.h, self.qn, self.I, self.qkv_n, self.nh, self.nkv, self.hd))
        # the same segment for 2..30 token rows (csrc/tree_segment.hip): attention + ONE resident launch per layer instead of 7
        # launches.  Measured on MI355X at the 1B draft's geometry (profiles/r05_tree_seg_probe_v1.txt, parity tests/test_hip_tree_segment.py):
        # the K+1 = 8-row glue decode 0.945 -> 0.857 ms (kept), the 24-row tree step 0.943 -> 0.965 ms (NOT kept: at 24 rows every
        # all-to-all edge costs ~4.5 us of flag latency + ~5 us to read 96-192 KB of freshly written rows in every workgroup -- what the
        # six kernel boundaries it replaces cost).  "auto" = on at that geometry for forwards of 2..16 rows;
        # 1 = every shape and row count the kernel accepts (tests); 0 = off.
        _ts = os.environ.get("SSD_TREE_SEG", "auto")
        self.tree_seg_rows = 32 if _ts == "1" else 16
        self.tree_seg_colocated = False     # set by the engine for a draft server that shares its GPU with the target (llm_engine.py)
        # (a q / k norm model -- Qwen3-0.6B, the draft of BASELINE configs[4] -- leaves the segment with raw QKV rows; the norm + RoPE +
        #  KV store stay with ssd_rope_store_kv in front of the attention launch: 3 launches per layer instead of 8.  Parity-green at
        #  that geometry (tests/test_hip_tree_segment.py) but NOT faster -- a 0.6B layer streams 15 MB, so the segment's fixed edge cost
        #  is all there is: tree step 1.248 -> 1.240 ms at 6 rows, 1.275 -> 1.299 at 12, 1.363 -> 1.457 at 24,
        #  profiles/r05_tree_seg_probe_qwen.txt -- so "auto" leaves it off there)
        self.tree_seg = ((_ts == "1" or (_ts == "auto" and _validated)) and tp_size == 1 and not self.use_coll and not self.quantized
                         and not self.moe and not self.kv8 and taps is None and max_tokens >= 2
                         and H.tree_segment_ok(2, self.h, self.qn, self.I, self.qkv_n, self.nh, self.nkv, self.hd))
        if self.chain_seg:
            self.chain_gr = z(H.chain_granule_bytes(self.h, self.I) // 8, dtype=torch.int64)
            self.buf_res3 = z(1, self.h)             # the chain's residual ping-pongs between buf_res2 and this (every workgroup re-reads res_in)
        if self.chain_seg or self.tree_seg:
            self.chain_gen = z(1, dtype=torch.int32)
            self.chain_err = z(1, dtype=torch.int32)
        if self.tree_seg:
            self.tree_ws = z(H.tree_segment_workspace_bytes(self.h, self.I) // 8, dtype=torch.int64)
            self.buf_res_b = z(min(T, 32), self.h)        # the residual ping-pongs: every workgroup re-reads a layer's input residual
        self._last: Slabs | None = None     # the last forward()'s hand-off, for the compute_logits that follows it
        pt = min(T, 32)
        self.buf_parts_o = z(16 * pt * self.h, dtype=torch.float32) if self.use_parts else None
        self.buf_parts_d = z(16 * pt * self.h, dtype=torch.float32) if self.use_parts else None
        self.logits = z(self.max_logit_rows, self.V)
        # EAGLE-3 target (ssd/models/llama3.py:256-271): the residual stream ENTERING the tapped layers (bf16(hidden + residual),
        # = the residual the layer's input add+norm writes anyway), concatenated in layer order for the draft's fc
        self.taps = sorted(set(taps)) if taps else None
        self.acts = z(T, len(self.taps) * self.h) if self.taps else None
        self.max_splits = 16
        # fp32 split-K partials of the prefill GEMM (csrc/gemm_pf.hip), sized ONCE for the largest matrix that can take that
        # path (layer matrices and the LM head): prefill hipGraphs bake this pointer, so it must never be reallocated
        pf_shapes = [(self.qkv_n, self.h), (self.h, self.qn), (2 * self.I, self.h), (self.h, self.I), (self.V, self.h)]
        if self.moe:        # the router is the one MLP matrix of a MoE layer that runs on the dense GEMMs
            self.moe_En = -(-cfg.num_experts // 16) * 16        # its rows padded to whole 16-row groups (zero rows: logits never read)
            pf_shapes[2:4] = [(self.moe_En, self.h)]
        need = max([H.gemm_pf_workspace_bytes(128, n, k) // 4 for n, k in pf_shapes if self._pf_eligible(n, k)], default=0)
        # a whole prompt of >= LM_MIN_TOKENS rows is one gemm_pf launch per linear, whatever the matrix size; the query at
        # max_tokens covers every shorter prompt (0 where no decomposition splits K)
        self._lm_ok = max_tokens > 128
        if self._lm_ok:
            need = max([need] + [self._lm_ws_numel(n, k) for n, k in pf_shapes])
        self._ws_pf = z(max(need, 1), dtype=torch.float32) if (need or self._lm_ok) and max_tokens > 32 else None
        # fp8 prompts longer than FP8_DIRECT_MAX_T rows: each matrix is dequantized into this bf16 fragment-major scratch, then runs on
        # the bf16 prefill GEMMs (compute-bound there, so the halved weight bytes buy nothing).  Allocated once: prefill hipGraphs
        # bake its pointer.
        # The same scratch serves w4a16 prompts longer than W4_DIRECT_MAX_T rows.
        # ... and mxfp4 prompts longer than MX4_DIRECT_MAX_T rows.
        direct_max = self.W4_DIRECT_MAX_T if self.w4 else self.MX4_DIRECT_MAX_T if self.mx4 else self.FP8_DIRECT_MAX_T
        self._deq = (z(max(n * k for n, k in pf_shapes[:4])) if self.quantized and max_tokens > direct_max else None)
        st = min(T, max_split_tokens)
        self.ws_o = z(st * self.nh * self.max_splits * self.hd, dtype=torch.float32)
        self.ws_ml = z(st * self.nh * self.max_splits * 2, dtype=torch.float32)
        # LM-head argmax candidates (csrc/gemm.hip EPI_ROWS_ARGMAX): one (value, index) per token row and workgroup, finished
        # by ssd_argmax_parts* -- on the greedy path for up to 32 logit rows (decode / verify / tree step)
        self.argmax_fused = True
        self.ap_rows = min(self.max_logit_rows, 32)
        self.ap_stride = max(H.gemm_argmax_nparts(m, self.V, self.h) for m in ({1, self.ap_rows} if self.ap_rows > 16 else {1}))
        self.ap_val = z(self.ap_rows, self.ap_stride, dtype=torch.float32)
        self.ap_idx = z(self.ap_rows, self.ap_stride, dtype=torch.int32)
        # (whether candidates exist for n rows is a function of n alone -- never of Python-side state, which a hipGraph replay
        #  of compute_logits would not update)
        # vocab-parallel argmax scratch
        self.am_val = z(tp_size, self.max_logit_rows, dtype=torch.float32)
        self.am_idx = z(tp_size, self.max_logit_rows, dtype=torch.int64)
        self.am_val_l = z(self.max_logit_rows, dtype=torch.float32)
        self.am_idx_l = z(self.max_logit_rows, dtype=torch.int64)
        # packed form for the one-shot exchange: per rank [R int64 indices | R fp32 values (+ pad to 8 bytes)]
        self.am_words = self.max_logit_rows + (self.max_logit_rows + 1) // 2
        self.am_pack_l = z(self.am_words, dtype=torch.int64)
        self.am_pack = z(tp_size, self.am_words, dtype=torch.int64)
        if max_loras:
            self._alloc_lora(z)
        if self.moe:
            self._alloc_moe(z)

    # ---- routed experts ------------------------------------------------------------------------------
    def _alloc_moe(self, z) -> None:
        """Everything a MoE layer writes between its norm and the combine, once (hipGraphs bake the pointers): the normed rows (the
        grouped GEMM gathers row-major x), the router-logit rows, the route tables, and act / d by entry (entry = token * k + choice)."""
        cfg, T = self.cfg, self.max_tokens
        E, k = cfg.num_experts, cfg.num_experts_per_tok
        self.moe_x = z(T, self.h)
        self.moe_logits = z(T, self.moe_En)
        self.moe_ids = z(T * k, dtype=torch.int32)
        self.moe_w = z(T * k, dtype=torch.float32)
        self.moe_offs = z(E + 1, dtype=torch.int32)
        self.moe_perm = z(T * k, dtype=torch.int32)
        self.moe_act = z(T * k, self.I)
        self.moe_d = z(T * k, self.h)

    def _load_moe(self, name: str, w: torch.Tensor) -> bool:
        """The three tensors of a MoE layer's MLP -> their device tables; False for any other name."""
        from ssd_amd.weights import MOE_GATE, MOE_GATE_UP, MOE_DOWN
        E = self.cfg.num_experts
        if name.endswith(MOE_GATE):             # the router: fragment-major, zero rows up to a whole 16-row group
            assert tuple(w.shape) == (E, self.h), (name, tuple(w.shape))
            pad = torch.zeros(self.moe_En, self.h, dtype=BF16, device=self.device)
            pad[:E] = w
            out = torch.empty(self.moe_En * self.h, dtype=BF16, device=self.device)
            H.rows_to_frag(pad, out, self.moe_En, self.h)
        elif name.endswith(MOE_GATE_UP) or name.endswith(MOE_DOWN):
            # E matrices, one after the other, each fragment-major; gate_up with gate / up 16-row groups interleaved (mode 1)
            up = name.endswith(MOE_GATE_UP)
            N, K = (2 * self.I, self.h) if up else (self.h, self.I)
            assert tuple(w.shape) == (E, N, K), (name, tuple(w.shape))
            out = torch.empty(E * N * K, dtype=BF16, device=self.device)
            for e in range(E):
                H.rows_to_frag(w[e], out[e * N * K:(e + 1) * N * K], N, K, mode=1 if up else 0)
        else:
            return False
        self.w[name] = out
        return True

    def _moe_up(self, li: int, T: int) -> None:
        """The normed rows are in moe_x (rows) and buf_xf (frag): router GEMM -> route -> grouped gate_up GEMM with SiLU * mul."""
        from ssd_amd.weights import MOE_GATE, MOE_GATE_UP
        cfg, p = self.cfg, f"model.layers.{li}."
        E, k = cfg.num_experts, cfg.num_experts_per_tok
        self._gemm(self.buf_xf, self.h, self.w[p + MOE_GATE], self.moe_En, self.moe_logits, T, self.moe_En)
        MOE.moe_route(self.moe_logits, self.moe_En, T, E, k, cfg.norm_topk_prob, self.moe_ids, self.moe_w, self.moe_offs, self.moe_perm)
        if self.moe_trace is not None:
            self.moe_trace.append((self.moe_logits[:T, :E].cpu(), self.moe_ids[:T * k].view(T, k).cpu()))
        MOE.moe_gemm(self.moe_x, self.w[p + MOE_GATE_UP], self.moe_offs, self.moe_perm, self.moe_act, T, k, E, 2 * self.I, self.h,
                     MOE.EPI_UP)

    def _moe_down(self, li: int, T: int) -> None:
        """Grouped down GEMM of moe_act -> moe_d by entry, then the weighted combine into buf_h (rows: the hand-off None)."""
        from ssd_amd.weights import MOE_DOWN
        cfg = self.cfg
        E, k = cfg.num_experts, cfg.num_experts_per_tok
        MOE.moe_gemm(self.moe_act, self.w[f"model.layers.{li}." + MOE_DOWN], self.moe_offs, self.moe_perm, self.moe_d, T, k, E, self.h,
                     self.I, MOE.EPI_DOWN)
        MOE.moe_combine(self.moe_d, self.moe_w, self.buf_h, T, k, self.h)

    # ---- LoRA adapters -----------------------------------------------------------------------------
    LORA_SPLIT_MAX_T = 256      # forwards of up to this many rows split the shrink's K over the default number of workgroups; longer
                                # (prefill-sized) ones have the rows to fill the chip and keep one slab

    def _alloc_lora(self, z) -> None:
        """Everything the adapted route needs, once: the slot tables per layer and linear (their pointers are baked into hipGraphs),
        the scale table, the row_slot array, the shrink workspace, and bf16 rows [max_tokens][2 I] for gate_up, which otherwise
        never exists as rows (1.9 GB at the 70B shapes with 16384 rows)."""
        cfg, S, T = self.cfg, self.max_loras, self.max_tokens
        self.lora_geo = {lin: LR.linear_shape(lin, cfg) + (LR.slot_rank(lin, self.max_lora_rank),) for lin in LR.LINEARS}   # (N, K, R)
        self.lora_a = {(li, lin): z(S * R * K) for li in range(cfg.num_layers) for lin, (N, K, R) in self.lora_geo.items()}
        self.lora_b = {(li, lin): z(S * N * R) for li in range(cfg.num_layers) for lin, (N, K, R) in self.lora_geo.items()}
        self.lora_scale = z(S, dtype=torch.float32)
        self.lora_rows = torch.full((T,), -1, dtype=torch.int32, device=self.device)
        Rmax = max(R for _, _, R in self.lora_geo.values())
        self.lora_ws = z(max(LO.MAX_SPLITS * min(T, self.LORA_SPLIT_MAX_T), T) * Rmax, dtype=torch.float32)
        self.buf_gu = z(T, 2 * self.I)

    def lora_bytes(self) -> int:
        """Device bytes the adapter support takes beside the weights (0 without it)."""
        if not self.max_loras:
            return 0
        ts = list(self.lora_a.values()) + list(self.lora_b.values()) + [self.lora_scale, self.lora_rows, self.lora_ws, self.buf_gu]
        return sum(t.numel() * t.element_size() for t in ts)

    def set_lora(self, slot: int, adapter) -> None:
        """Copy a ssd_amd.lora.LoraAdapter into slot `slot` of every table (packed per fused linear, zero-padded to the slot's rank,
        re-tiled fragment-major) and set the slot's scale.  Adapters are data: the graphs that ran another adapter run this one."""
        assert 0 <= slot < self.max_loras
        for (li, lin), a_tab in self.lora_a.items():
            N, K, R = self.lora_geo[lin]
            A, B = LR.pack_linear(adapter, li, lin, self.cfg, R)
            H.rows_to_frag(A.to(self.device), a_tab[slot * R * K:(slot + 1) * R * K], R, K)
            H.rows_to_frag(B.to(self.device), self.lora_b[(li, lin)][slot * N * R:(slot + 1) * N * R], N, R)
        self.lora_scale[slot] = adapter.scale
        torch.cuda.synchronize(self.device)

    def clear_lora(self, slot: int) -> None:
        assert 0 <= slot < self.max_loras
        for (li, lin), a_tab in self.lora_a.items():
            N, K, R = self.lora_geo[lin]
            a_tab[slot * R * K:(slot + 1) * R * K].zero_()
            self.lora_b[(li, lin)][slot * N * R:(slot + 1) * N * R].zero_()
        self.lora_scale[slot] = 0.0
        torch.cuda.synchronize(self.device)

    def _lora_delta(self, li: int, lin: str, xf, y, T: int, ldy: int, act_frag=None) -> None:
        """shrink + expand of layer li's linear `lin` on the rows y its GEMM has just stored from the activations xf."""
        N, K, R = self.lora_geo[lin]
        S = 0 if T <= self.LORA_SPLIT_MAX_T else 1
        LO.lora_shrink(xf, self.lora_a[(li, lin)], self.lora_rows, self.lora_ws, T, K, R, self.max_loras, S)
        LO.lora_expand(self.lora_ws, self.lora_b[(li, lin)], self.lora_scale, self.lora_rows, y, ldy, T, N, K, R, self.max_loras, S,
                       LO.EPI_ADD if act_frag is None else LO.EPI_SILU, act_frag)

    # ---------------------------------------------------------------------------------------------
    def load_weights(self, weight_iter) -> None:
        """Consumes (name, row-major bf16 shard) pairs; matrices are re-tiled once into the fragment-major layout (gate_up with
        gate/up row groups interleaved for the fused SiLU epilogue).  A decoder linear may also come pre-quantized, as one of the
        host forms of ssd_amd/quant.py (a plain (q, s) pair is a quant.FP8Tensor).  The rule: a quantized decoder packs a linear of
        its own kind as it is, "<name>" = frag codes plus the "<name>_scale" / "_zero" / "_bscale" tables of that form (_load_fp8,
        _load_w4, _load_mx4), quantizes a bf16 linear as it arrives (never the whole model in both forms) and refuses a linear of
        another kind; everything else -- any host form into a bf16 decoder, embeddings, LM head, norms -- loads as bf16, a host
        form as the exact dequantized matrix."""
        kind = self._kind()
        for name, w in weight_iter:
            if type(w) is tuple and len(w) == 2:
                w = quant.FP8Tensor(*w)
            if kind is not None and quant.is_quantized_linear(name):
                if not quant.is_prequantized(w):
                    w = self._quantize_on_load(w.to(self.device))
                elif w.native != kind:
                    raise ValueError(f"{name}: {w.phrase} tensors cannot load into a {kind} decoder")
                self._load_quantized(name, quant.to_device(w, self.device))
                continue
            if quant.is_prequantized(w):        # a bf16 decoder (or a matrix that stays bf16) computes with bf16(s * q)
                w = quant.to_device(w, self.device).dequantize()
            w = w.to(self.device).contiguous()
            if self.moe and self._load_moe(name, w):
                continue
            if name.endswith("qkv_proj.weight"):
                # rotation-paired row order: RoPE pairs share an accumulator tile (fused epilogue) -- layout.hip
                out = torch.empty(w.numel(), dtype=BF16, device=self.device)
                H.rows_to_frag_qkv(w, out, self.nh, self.nkv, self.hd, w.shape[1])
                self.w[name] = out
            elif name.endswith("qkv_proj.bias"):
                self.w[name] = w[self._qkv_row_perm().to(self.device)].contiguous()
            elif w.dim() == 2 and not name.endswith("embed_tokens.weight"):
                R, K = w.shape
                out = torch.empty(H.frag_numel(R, K), dtype=BF16, device=self.device)
                H.rows_to_frag(w, out, R, K, mode=1 if name.endswith("gate_up_proj.weight") else 0)
                self.w[name] = out
            elif name.endswith("embed_tokens.weight"):
                self.w[name] = w                                   # row-major for the gather
                if self.cfg.tie_word_embeddings:                   # tied LM head: same values, GEMM layout
                    out = torch.empty(H.frag_numel(w.shape[0], w.shape[1]), dtype=BF16, device=self.device)
                    H.rows_to_frag(w, out, w.shape[0], w.shape[1])
                    self.w["lm_head.weight"] = out
            else:
                self.w[name] = w
        torch.cuda.synchronize(self.device)

    def _kind(self) -> str | None:
        """The `quantization` value this decoder runs, read off its flags."""
        return "fp8" if self.fp8 else "w4a16" if self.w4 else "mxfp4" if self.mx4 else None

    def _quantize_on_load(self, w: torch.Tensor):
        """The host form this decoder's own quantizer gives a bf16 linear."""
        if self.fp8:
            return quant.quantize_fp8(w)
        if self.mx4:
            return quant.quantize_mxfp4(w)
        return quant.quantize_w4a16_zp(w) if self.w4_zero_point else quant.quantize_w4a16(w)

    def _load_quantized(self, name: str, w) -> None:
        """A host form of this decoder's kind, on the device -> its codes and side tables in the packed row order (QKV: rotation-
        paired, gate_up: interleaved), stored under "<name>" + the suffixes the format's loader answers with."""
        N, K = w.shape()
        row_map = None
        if name.endswith("qkv_proj.weight"):
            row_map = quant.qkv_row_map(self.nh, self.nkv, self.hd).to(self.device)
        elif name.endswith("gate_up_proj.weight"):
            row_map = quant.gate_up_row_map(N).to(self.device)
        load = self._load_fp8 if self.fp8 else self._load_mx4 if self.mx4 else self._load_w4
        for suffix, t in load(name, w, N, K, row_map).items():
            self.w[name + suffix] = t

    def _frag(self, numel: int, dtype) -> torch.Tensor:
        return torch.empty(numel, dtype=dtype, device=self.device)

    def _load_fp8(self, name: str, w, N: int, K: int, row_map) -> dict:
        """FP8Tensor -> fp8 frag codes + "_scale" fp32 [N]; FP8BTensor -> the same codes + "_bscale" fp32 [N / 16, ceil(K / 128)], one
        scale per 16-row group and column block (include/ssd_hip_fp8b.h).  A linear has one or the other."""
        block = isinstance(w, quant.FP8BTensor)
        s = w.rowscale.to(torch.float32).contiguous() if block else w.scale.to(torch.float32).reshape(-1).contiguous()
        assert w.codes.dtype == quant.FP8 and tuple(s.shape) == ((N, -(-K // quant.FP8_BLOCK)) if block else (N,)), (name, w.codes.dtype, s.shape)
        codes = self._frag(N * K, torch.uint8)
        Q.fp8_rows_to_frag(w.codes.contiguous().view(torch.uint8), codes, N, K, row_map=row_map)
        if block:
            return {"": codes, "_bscale": quant.fp8_block_group_scales(s, row_map, name)}
        return {"": codes, "_scale": s if row_map is None else s[row_map.long()].contiguous()}

    def _load_w4(self, name: str, w, N: int, K: int, row_map) -> dict:
        """W4Tensor -> w4 frag codes + "_scale" bf16 frag scales (include/ssd_hip_w4a16.h); W4ZTensor -> those + "_zero", the zero-point
        table (include/ssd_hip_w4zp.h)."""
        packed, s = w.packed.contiguous(), w.scale.to(BF16).contiguous()
        assert packed.dtype == torch.int32 and tuple(s.shape) == (N, K // quant.W4_GROUP), (name, packed.dtype, s.shape)
        out = {"": self._frag(N * K // 2, torch.uint8), "_scale": self._frag(N * K // quant.W4_GROUP, BF16)}
        if isinstance(w, quant.W4ZTensor):
            zero = w.zero.contiguous()
            assert zero.dtype == torch.uint8 and zero.shape == s.shape and int(zero.max()) <= 15, (name, zero.dtype, zero.shape)
            out["_zero"] = self._frag(N * K // quant.W4_GROUP, torch.uint8)
            W4Z.w4zp_rows_to_frag(packed, s, zero, out[""], out["_scale"], out["_zero"], N, K, row_map=row_map)
        else:
            W4.w4_rows_to_frag(packed, s, out[""], out["_scale"], N, K, row_map=row_map)
        return out

    def _load_mx4(self, name: str, w, N: int, K: int, row_map) -> dict:
        """MX4Tensor -> mx4 frag codes + "_scale" mx4 frag scale bytes (include/ssd_hip_mxfp4.h)."""
        packed, s = w.packed.contiguous(), w.scale.contiguous()
        assert packed.dtype == torch.uint8 and tuple(s.shape) == (N, K // quant.MX4_BLOCK), (name, packed.dtype, s.shape)
        quant.check_mxfp4_scales(name, s)
        out = {"": self._frag(N * K // 2, torch.uint8), "_scale": self._frag(N * K // quant.MX4_BLOCK, torch.uint8)}
        MX4.mx4_rows_to_frag(packed, s, out[""], out["_scale"], N, K, row_map=row_map)
        return out

    def overwrite_weights(self, weight_iter) -> None:
        """New VALUES into the existing weight tensors (same names and shapes): captured hipGraphs keep pointing at the same memory, so a
        model can be given other weights without recapturing anything (bench.py: the independent-draft leg after the correlated one)."""
        old, self.w = self.w, {}
        self.load_weights(weight_iter)
        new, self.w = self.w, old
        assert set(new) == set(old), sorted(set(new) ^ set(old))
        for n, t in new.items():
            old[n].copy_(t)
        torch.cuda.synchronize(self.device)

    def _qkv_row_perm(self) -> torch.Tensor:
        """quant.qkv_row_map as an index tensor: the order the bf16 QKV bias is permuted with."""
        return quant.qkv_row_map(self.nh, self.nkv, self.hd).long()

    def weight_bytes(self) -> int:
        """HBM bytes one forward must stream (every matrix once; the embedding table is only gathered; fp8 or int4 codes + their
        scales)."""
        return sum(t.numel() * t.element_size() for n, t in self.w.items() if n != "model.embed_tokens.weight")

    def kv_block_bytes(self) -> int:
        return 2 * self.cfg.num_layers * self.block_size * self.nkv * self.hd * (1 if self.kv8 else 2)

    def alloc_kv(self, num_blocks: int) -> None:
        # [L][2][blocks][nkv][block_size][hd]: one (page, kv head) is a contiguous run for the attention kernel
        self.num_blocks = num_blocks
        self.kv_cache = torch.zeros(self.cfg.num_layers, 2, num_blocks, self.nkv, self.block_size, self.hd,
                                    dtype=torch.uint8 if self.kv8 else BF16, device=self.device)

    def set_kv_scales(self, k_scale: torch.Tensor, v_scale: torch.Tensor) -> None:
        """fp8 KV cache: per layer and kv head scales, fp32 [L, nkv] each (positive, finite).  Copied INTO the device tables (their
        pointers are baked into hipGraphs); the inverse the store multiplies by is computed here in fp32.  Codes already in the
        cache keep the scale they were stored with: set the scales before the first forward."""
        if not self.kv8:
            raise ValueError("set_kv_scales needs kv_cache_dtype='fp8'")
        L = self.cfg.num_layers
        ks = torch.as_tensor(k_scale, dtype=torch.float32).reshape(L, self.nkv)
        vs = torch.as_tensor(v_scale, dtype=torch.float32).reshape(L, self.nkv)
        s = torch.stack([ks, vs], dim=1)
        if not (torch.isfinite(s).all() and (s > 0).all()):
            raise ValueError("KV scales must be positive and finite")
        self.kv_scale.copy_(s)
        self.kv_inv_scale.copy_(1.0 / s)

    def _attn(self, li: int, T: int, meta: AttnMeta, splits: int, flags: int | None, waves: int, scale: float) -> None:
        """The layer's paged attention launch into buf_af, over the bf16 or the fp8 cache.  flags None: left to the kernel's default
        (0: the chain / tree segments and the EAGLE-3 draft, which never take forward()'s _attn_flags)."""
        fl = {} if flags is None else dict(flags=flags)
        if self.kv8:
            assert meta.mode == H.MODE_CAUSAL, "the fp8 KV cache serves the target's causal shapes only"
            KV8.attn_paged_fp8(self.buf_q, self.kv_cache[li, 0], self.kv_cache[li, 1], meta.block_tables, self.max_blocks,
                               meta.context_lens, meta.B, T, meta.max_q, self.nh, self.nkv, self.hd, self.block_size, scale,
                               k_scale=self.kv_scale[li, 0], v_scale=self.kv_scale[li, 1], cu_q=meta.cu_q, q_per_seq=meta.q_per_seq,
                               splits=splits, ws_o=self.ws_o, ws_ml=self.ws_ml, out_frag=self.buf_af, waves=waves, **fl)
            return
        H.attn_paged(self.buf_q, self.kv_cache[li, 0], self.kv_cache[li, 1], meta.block_tables, self.max_blocks,
                     meta.context_lens, meta.B, T, meta.max_q, self.nh, self.nkv, self.hd, self.block_size, scale,
                     cu_q=meta.cu_q, q_per_seq=meta.q_per_seq, mode=meta.mode, tree_K=meta.tree_K, tree_mq=meta.tree_mq,
                     tree_step=meta.tree_step, tree_F=meta.tree_F, tree_jidx=meta.tree_jidx, splits=splits,
                     ws_o=self.ws_o, ws_ml=self.ws_ml, out_frag=self.buf_af, waves=waves, **fl)

    # ---------------------------------------------------------------------------------------------
    PF_MIN_WEIGHT_BYTES = 100 << 20

    @classmethod
    def _pf_eligible(cls, N: int, K: int) -> bool:
        return 2 * N * K >= cls.PF_MIN_WEIGHT_BYTES and N % 128 == 0 and K % 128 == 0

    # prompts of at least this many rows run every linear as ONE long-prefill GEMM launch (csrc/gemm_pf.hip gemm_lm_kernel,
    # compute-bound) instead of a loop of 128-row chunks that re-streams the weights once per chunk
    LM_MIN_TOKENS = 256
    LM_MAX_TOKENS = 16384
    # fp8 linears of up to this many rows run on the fp8 GEMM itself; longer prompts dequantize into self._deq first
    FP8_DIRECT_MAX_T = 128
    # w4a16 linears of up to this many rows run on the w4a16 GEMM itself; longer prompts dequantize into self._deq first
    W4_DIRECT_MAX_T = 128
    # mxfp4 linears of up to this many rows run on the mxfp4 GEMM itself; longer prompts dequantize into self._deq first
    MX4_DIRECT_MAX_T = 128

    @classmethod
    def _lm_eligible(cls, T: int) -> bool:
        return cls.LM_MIN_TOKENS <= T <= cls.LM_MAX_TOKENS

    def _lm_ws_numel(self, N: int, K: int) -> int:
        """fp32 workspace elements the long-prefill GEMM of an N x K matrix needs for any prompt up to max_tokens rows."""
        if N % 128 or K % 128:
            return 0
        return H.gemm_pf_workspace_bytes(min(self.max_tokens, self.LM_MAX_TOKENS), N, K) // 4

    def _gemm_chunk(self, xf, K, w, N, y, m, ldy, epi, bias):
        """One <= 128-row chunk.  Prefill-sized chunks of a big matrix go to the LDS-shared / split-K kernel
        (csrc/gemm_pf.hip): measured on MI355X at M = 128, 70B layer GEMMs 611 -> 383 us, 8B gate_up 83 -> 62 us; small
        matrices (<100 MB: too few workgroups without deep K-splits) stay on the skinny kernel."""
        if m > 32 and self._pf_eligible(N, K):
            assert self._ws_pf is not None and self._ws_pf.numel() * 4 >= H.gemm_pf_workspace_bytes(128, N, K), (N, K)
            H.gemm_pf(xf, w, y, m, N, K, ldy, self._ws_pf, epilogue=epi, bias=bias)
        else:
            H.gemm(xf, w, y, m, N, K, ldy, epi, bias)

    def _pf_partials_ok(self, T: int, N: int, K: int) -> bool:
        """o_proj / down_proj of ONE prefill chunk may leave their split-K partials in the workspace for the norm that follows."""
        return self.pf_parts and not self.use_coll and 32 < T <= 128 and self._pf_eligible(N, K) and self._ws_pf is not None

    def _gemm_pf_partials(self, xf, K, w, N, T, min_splits: int = 1) -> Slabs | None:
        """Prefill GEMM stopped after its split-K stage (csrc/gemm_pf.hip PF_EPI_PARTIALS): fp32 slabs [S][T][N] in the workspace, summed
        by the consumer (ssd_rmsnorm_parts / ssd_rope_store_kv_parts) -- one launch per GEMM less.  Nothing is launched, and None
        returned, where the decomposition has fewer than min_splits slabs."""
        S = H.gemm_pf_workspace_bytes(T, N, K) // (4 * T * N)
        if S < min_splits:
            return None
        H.gemm_pf(xf, w, None, T, N, K, N, self._ws_pf, epilogue=H.PF_EPI_PARTIALS)
        return Slabs(self._ws_pf, S, T)

    def _quant_route(self, name: str):
        """(GEMM, dequantizer, direct limit, side tables) of a quantized linear, chosen by the tables load_weights left beside its
        codes; None for a bf16 matrix.  The ops are read off their modules at every call: a trace or a probe may have replaced them."""
        scale, bscale = self.w.get(name + "_scale"), self.w.get(name + "_bscale")
        if bscale is not None:          # fp8 codes + block scales per 16-row group (a linear has these or row scales, never both)
            assert scale is None and self.fp8
            return F8B.gemm_fp8b, F8B.fp8b_dequant_frag, self.FP8_DIRECT_MAX_T, (bscale,)
        if scale is None:
            return None
        if self.w4:                     # w4a16 codes + group scales, and group zero points where the linear has them
            zero = self.w.get(name + "_zero")
            if zero is not None:
                return W4Z.gemm_w4a16_zp, W4Z.w4zp_dequant_frag, self.W4_DIRECT_MAX_T, (scale, zero)
            return W4.gemm_w4a16, W4.w4_dequant_frag, self.W4_DIRECT_MAX_T, (scale,)
        if self.mx4:                    # mxfp4 codes + block scale bytes
            return MX4.gemm_mxfp4, MX4.mx4_dequant_frag, self.MX4_DIRECT_MAX_T, (scale,)
        return Q.gemm_fp8, Q.fp8_dequant_frag, self.FP8_DIRECT_MAX_T, (scale,)      # fp8 codes + row scales

    def _gemm(self, xf, K, w, N, y, T, ldy, epi=H.EPI_ROWS, bias=None):
        """y = xf @ w^T.  w is a fragment-major bf16 matrix, or the name of a decoder linear in self.w: a quantized one runs on its
        format's GEMM up to that format's direct limit of rows and is dequantized into self._deq for the bf16 routes beyond it."""
        if isinstance(w, str):
            route, w = self._quant_route(w), self.w[w]
            if route is not None:
                gemm, dequant, direct_max, side = route
                if T <= direct_max:
                    gemm(xf, w, *side, y, T, N, K, ldy, epi, bias)
                    return
                dequant(w, *side, self._deq, N, K)
                w = self._deq
        if T > 128 and self._lm_eligible(T) and N % 128 == 0 and K % 128 == 0:
            assert self._ws_pf is not None and self._ws_pf.numel() * 4 >= H.gemm_pf_workspace_bytes(T, N, K), (T, N, K)
            H.gemm_pf(xf, w, y, T, N, K, ldy, self._ws_pf, epilogue=epi, bias=bias)
            return
        if T <= 128:
            self._gemm_chunk(xf, K, w, N, y, T, ldy, epi, bias)
            return
        yf = y.view(-1)
        for m0 in range(0, T, 128):
            m = min(128, T - m0)
            x_off = (m0 // 16) * (K // 32) * 512
            y_off = (m0 // 16) * ((N // 2) // 32) * 512 if epi == H.EPI_SILU_FRAG else m0 * ldy
            self._gemm_chunk(xf[x_off:], K, w, N, yf[y_off:], m, ldy, epi, bias)

    def _allreduce(self, t):
        if not self.use_coll:
            return
        if self.custom_ar is not None and self.custom_ar.fits(t):
            self.custom_ar.all_reduce(t)        # one-shot full-mesh sum over xGMI (csrc/comm.hip)
        else:
            dist.all_reduce(t, group=self.tp_group)

    @staticmethod
    def ctx_bucket(ctx: int) -> int:
        """Power-of-two context bucket (>= 1024): the attention decomposition is static per hipGraph, and up to
        1024 keys a single workgroup per (sequence, kv head) with no merge kernel is the fastest one."""
        b = 1024
        while b < ctx:
            b *= 2
        return b

    def _attn_cfg(self, T: int, meta: AttnMeta) -> tuple[int, int]:
        """(grid key-splits, waves per workgroup).  Up to 8 waves of one workgroup split the key range and merge
        in LDS (one launch).  A decode-side launch occupies only B*nkv*row_tiles CUs and each CU sustains a few
        tens of GB/s of K/V loads, so beyond ~1K keys per workgroup the scan is spread over more workgroups with
        grid key-splits + the merge kernel (measured on MI355X, 1B decode: ctx 2048 22 -> 13 us, 4096 39 -> 17 us;
        below 1K keys the extra launch costs more than it saves)."""
        G = self.nh // self.nkv
        row_tiles = -(-(meta.max_q * G) // 16)
        # attn_launch's default of two row tiles per workgroup above 8 tiles.  _attn_flags launches those shapes with ONE tile per
        # workgroup, so the real grid is twice this model's; the two-tile model is kept on purpose: it decides the wave split, and with
        # the wave split the accumulation order -- the bit pattern -- of every prefill stays what it is
        groups = -(-row_tiles // 2) if row_tiles > 8 else row_tiles
        base = max(1, groups * meta.B * self.nkv)
        waves = max(1, min(8, 512 // base))
        # (prefill with 4 / 8 waves per workgroup, measured on c4: TTFT 30.92 ms (this heuristic, 2 waves) / 30.68 / 30.74 -- within noise, and
        #  another accumulation order: not adopted, the override switch retired in round 5)
        ctx = self.ctx_bucket(meta.ctx_hint if meta.ctx_hint > 0 else self.max_model_len)
        splits = 1 if ctx <= 1024 else max(1, min(self.max_splits, ctx // 512))
        if base >= 256 or T > self.max_split_tokens:
            splits = 1
        return splits, waves

    def _attn_flags(self, meta: AttnMeta) -> int:
        """ssd_attn_paged flags.  Query blocks of more than 8 row tiles per kv head (prefill chunks) take ONE 16-row tile per workgroup
        (bit 2) instead of the kernel's default two: twice the workgroups, K tiles prefetched (the two-tile variant of head_dim 128 has no
        registers for that) -- the same key split per wave, so bit-identical; measured at T = 128 (profiles/r06_prefill_small_kernels.txt):
        70B 17.0 -> 12.2 us, 8B 16.8 -> 10.6, 1B 12.4 -> 8.1; T = 512: 48.8 -> 46.6."""
        G = self.nh // self.nkv
        return 4 if -(-(meta.max_q * G) // 16) > 8 else 0

    @staticmethod
    def _parts_cfg(N: int, K: int, fused_consumer: bool = False) -> tuple[int, int]:
        """(K splits, waves) of the split-K partial-slab GEMM for a [N, K] matrix, from profiles/r02_draft_probe.txt (1B
        shapes, us per launch; rows kernel -> slabs): M = 1: o_proj 4.5 -> 3.7 (4 splits, 8 waves) / 3.9 (2, 16), down_proj
        10.0 -> 7.6 (4, 8) / 8.0 (2, 16); M = 24: 8.1 -> 4.2 and 16.7 -> 9.0.  Enough workgroups to put >= 2 on every CU and
        <= 8 k-tiles per wave, so that every wave has its whole share in flight at once.  When the consumer is the fused
        norm + GEMM prologue (every workgroup of the NEXT kernel re-reads the slabs) two slabs are the optimum: a third
        and fourth cost the consumers more than they save here."""
        groups, KT = N // 16, K // 32
        smax = 2 if fused_consumer else (16 if groups > 256 else 4)
        S = 1
        while groups * S < (5120 if groups > 256 else 512) and S < smax and KT // (S * 2) >= 8:
            S *= 2
        per = -(-KT // S)
        waves = 16 if fused_consumer else 8
        while waves < 16 and -(-per // waves) > 8:
            waves *= 2
        while waves > 2 and per // waves < 1:
            waves //= 2
        # a very long K: the kernel holds a wave's whole share in registers (<= 8 k-tiles).  More slabs where the consumer is a
        # stand-alone norm (up to the 16 the slab buffers hold); the two-slab fused consumer cannot take more -- __init__ then
        # keeps such a model on the rows kernels
        while not fused_consumer and S < 16 and -(-(-(-KT // S)) // waves) > 8:
            S *= 2
            waves = 16
        return S, waves

    def _parts(self, which: str, T: int) -> tuple[int, int]:
        fused = self.fusion_plan(T)[1]
        N, K = (self.h, self.qn) if which == "o" else (self.h, self.I)
        return self._parts_cfg(N, K, fused)

    def parts_plan(self, T: int) -> bool:
        """o_proj / down_proj as split-K partial slabs consumed by the next norm: single-rank models with < 256 row groups at
        decode-sized T (the draft's chain / glue / tree forwards)."""
        return self.use_parts and not self.use_coll and T <= 32

    def attn_o_plan(self, T: int, meta: AttnMeta, splits: int) -> bool:
        """Attention + o_proj as ONE launch (csrc/attention.hip OPROJ variant): single-rank models on the slab path, one
        sequence, causal decode rows, context scanned inside one workgroup (bucket <= 1024).  Only while the query rows of a
        kv head fit ONE 16-row tile (the single-token chain, up to 4 rows at G = 4): the N/128 workgroups of a head each
        repeat its attention, and with two row tiles (the K+1 = 8-row glue) that costs more than the saved launch --
        measured on the 1B draft (profiles/r03_draft_probe.txt): M = 1 forward 734 -> 718 us, M = 8 forward 838 -> 867 us.
        (Grouped-query models only, G >= 2: the shapes the kernel was validated at on the MI355X -- G = 4 and 2.)"""
        G = self.nh // self.nkv
        return (self.fuse_attn_o and self.parts_plan(T) and meta.mode == H.MODE_CAUSAL and meta.cu_q is None and meta.B == 1
                and splits == 1 and G >= 2 and T * G <= 16 and G * self.hd <= 256
                and self.h % 128 == 0 and self.nkv <= 16)

    # ---- the four GEMM launches of a layer (also used one by one by bench.py's roofline timing) ----
    def fusion_plan(self, T: int) -> tuple[bool, bool]:
        """(small, norm_fuse).  T <= 16: RoPE + KV store ride the QKV epilogue (csrc/gemm_fused.hip).  The residual
        add + RMSNorm ride the GEMM prologue only while M*K is tiny (single-token draft decode) and no all-reduce sits
        between producer and norm: the prologue is paid by EVERY workgroup and its LDS image limits residency --
        measured on MI355X, M=7 x K=4096 made gate_up 73 us vs 49 us unfused, M=1 x K=2048 made norm+qkv+rope 5.6 us
        vs 14.8 us."""
        small = T <= 16 and not self.cfg.qk_norm and not self.quantized and not self.kv8 and not self.moe
        return small, small and not self.use_coll and T * self.h // 8 <= 1024

    def chain_plan(self, T: int, meta: AttnMeta, splits: int) -> bool:
        """The resident single-token chain (csrc/chain.hip): one sequence, one new token, causal attention scanned inside one
        workgroup, the fused norm + QKV launch available for layer 0, no biases."""
        return (self.chain_seg and T == 1 and meta.B == 1 and meta.cu_q is None and meta.mode == H.MODE_CAUSAL and splits == 1
                and self.fusion_plan(T)[1] and "model.layers.0.self_attn.qkv_proj.bias" not in self.w)

    def _next_qkv(self, li: int, positions, meta: AttnMeta, rows: bool = False) -> dict:
        """What a chain / tree segment needs to run layer li's norm + QKV at its end: with RoPE + KV store, or (rows: the q / k norm
        models) leaving raw QKV rows in buf_qkv."""
        p = f"model.layers.{li}."
        nxt = dict(w_qkv_next=self.w[p + "self_attn.qkv_proj.weight"], ln_next=self.w[p + "input_layernorm.weight"])
        if rows:
            return dict(nxt, qkv_rows_next=self.buf_qkv)
        return dict(nxt, positions=positions, cos_sin=self.cos_sin, slots=meta.slot_mapping, q_out=self.buf_q,
                    k_cache=self.kv_cache[li, 0], v_cache=self.kv_cache[li, 1])

    def _forward_chain(self, positions, meta: AttnMeta, attn_waves: int) -> None:
        cfg, w = self.cfg, self.w
        L = cfg.num_layers
        scale = self.hd ** -0.5
        H.chain_tick(self.chain_gen)
        self.launch_qkv(0, 1, positions, meta.slot_mapping, src=None)       # layer 0: norm(embedding) + QKV + RoPE + KV store
        for li in range(L):
            self._attn(li, 1, meta, 1, None, attn_waves, scale)
            p = f"model.layers.{li}."
            last = li + 1 == L
            nxt = {} if last else self._next_qkv(li + 1, positions, meta)
            rin, rout = (self.buf_res2, self.buf_res3) if li % 2 == 0 else (self.buf_res3, self.buf_res2)
            H.chain_segment(self.buf_af, rin, self.buf_res if last else rout, w[p + "self_attn.o_proj.weight"],
                            w[p + "mlp.gate_up_proj.weight"], w[p + "mlp.down_proj.weight"], w[p + "post_attention_layernorm.weight"],
                            cfg.rms_norm_eps, self.h, self.qn, self.I, self.qkv_n, self.nh, self.nkv, self.hd, self.block_size, li,
                            self.chain_gr, self.chain_gen, self.chain_err, h_out=self.buf_h if last else None, **nxt)

    def tree_plan(self, T: int, meta: AttnMeta) -> bool:
        """The resident M-row layer segment (csrc/tree_segment.hip): decode-side forwards of 2..30 rows (tree steps, glue), no biases."""
        return (self.tree_seg and not self.tree_seg_colocated and 2 <= T <= self.tree_seg_rows and meta.cu_q is None and "model.layers.0.self_attn.qkv_proj.bias" not in self.w
                and H.tree_segment_ok(T, self.h, self.qn, self.I, self.qkv_n, self.nh, self.nkv, self.hd))

    def _forward_tree_seg(self, positions, T: int, meta: AttnMeta, splits: int, attn_waves: int) -> None:
        """embedding rows in buf_h -> [norm + QKV + RoPE + KV store of layer 0] -> per layer: attention, segment."""
        cfg, w = self.cfg, self.w
        L = cfg.num_layers
        scale = self.hd ** -0.5
        res = [self.buf_res, self.buf_res_b]
        start = L % 2               # layer li reads res[(start + li) % 2] and writes the other: the last layer's lands in buf_res
        H.chain_tick(self.chain_gen)
        H.rmsnorm(self.buf_h, w["model.layers.0.input_layernorm.weight"], cfg.rms_norm_eps, T, self.h, res_in=None, res_out=res[start],
                  out_frag=self.buf_xf)
        qk = cfg.qk_norm
        if qk:
            self._gemm(self.buf_xf, self.h, w["model.layers.0.self_attn.qkv_proj.weight"], self.qkv_n, self.buf_qkv, T, self.qkv_n)
        else:
            H.gemm_fused(w["model.layers.0.self_attn.qkv_proj.weight"], T, self.qkv_n, self.h, H.FEPI_QKV_ROPE, x_frag=self.buf_xf,
                         positions=positions, cos_sin=self.cos_sin, slots=meta.slot_mapping, q_out=self.buf_q, k_cache=self.kv_cache[0, 0],
                         v_cache=self.kv_cache[0, 1], nh=self.nh, nkv=self.nkv, hd=self.hd, block_size=self.block_size)
        for li in range(L):
            if qk:      # per-head q / k RMSNorm + RoPE + KV store of the rows the previous segment (or the GEMM above) left in buf_qkv
                p_ = f"model.layers.{li}.self_attn."
                H.rope_store_kv(self.buf_qkv, positions, self.cos_sin, meta.slot_mapping, self.buf_q, self.kv_cache[li, 0], self.kv_cache[li, 1],
                                T, self.nh, self.nkv, self.hd, self.block_size, q_norm_w=w[p_ + "q_norm.weight"],
                                k_norm_w=w[p_ + "k_norm.weight"], eps=cfg.rms_norm_eps, qkv_perm=1)
            self._attn(li, T, meta, splits, None, attn_waves, scale)       # (never forward()'s _attn_flags: not 0 at 24 rows with G = 16)
            p = f"model.layers.{li}."
            last = li + 1 == L
            nxt = {} if last else self._next_qkv(li + 1, positions, meta, rows=qk)
            H.tree_segment(self.buf_af, res[(start + li) % 2], res[(start + li + 1) % 2], w[p + "self_attn.o_proj.weight"],
                           w[p + "mlp.gate_up_proj.weight"], w[p + "mlp.down_proj.weight"], w[p + "post_attention_layernorm.weight"],
                           cfg.rms_norm_eps, T, self.h, self.qn, self.I, self.qkv_n, self.nh, self.nkv, self.hd, self.block_size, li,
                           self.tree_ws, self.chain_gen, self.chain_err, h_out=self.buf_h if last else None, **nxt)

    # ---- the hand-off between two launches: where the previous GEMM left the hidden state.  None = bf16 rows in buf_h, a Slabs = fp32
    # split-K slabs the consumer's norm sums, NORMED = the fused all-reduce + add + RMSNorm has already done the consumer's norm.
    # launch_o / launch_down (and the fused attention + o_proj) return it, launch_qkv / launch_gate_up take it as src=, forward()
    # threads it through the layers and keeps the last one for compute_logits.
    def _plan_src(self, which: str, T: int) -> Slabs | None:
        """The hand-off launch_o ("o") / launch_down ("d") leave at T rows when nobody says otherwise."""
        if not self.parts_plan(T):
            return None
        return Slabs(self.buf_parts_o if which == "o" else self.buf_parts_d, self._parts(which, T)[0], T)

    def _add_norm(self, src, T: int, weight, **kw) -> None:
        """Residual add + RMSNorm of the hidden state the hand-off `src` describes; kw: res_in / res_out / out_frag of the norm kernels,
        and gather (rows only), passed on as given."""
        if src is NORMED:
            return
        if src is None:
            H.rmsnorm(self.buf_h, weight, self.cfg.rms_norm_eps, T, self.h, **kw)
            return
        assert kw.pop("gather", None) is None and T == src.rows
        H.rmsnorm_parts(src.buf, src.n, src.rows, weight, self.cfg.rms_norm_eps, T, self.h, **kw)

    def _prologue_src(self, src) -> dict:
        """The same hand-off as the input of a norm-fused GEMM prologue (csrc/gemm_fused.hip)."""
        return dict(h_rows=self.buf_h) if src is None else dict(h_parts=src.buf, splits=src.n)

    def launch_qkv(self, li: int, T: int, positions, slot_mapping, gemm_only: bool = False, src=_PLAN) -> None:
        """gemm_only: skip the separate add+RMSNorm / RoPE launches of the unfused variants (kernel timing).
        src: the hand-off of the previous layer's down_proj (layer 0: None, the embedding rows)."""
        cfg, w = self.cfg, self.w
        p = f"model.layers.{li}."
        small, norm_fuse = self.fusion_plan(T)
        lora = self.lora_active
        if lora:            # the rows route: norm -> rows GEMM -> delta -> RoPE / KV store
            small = norm_fuse = False
        kc, vc = self.kv_cache[li, 0], self.kv_cache[li, 1]
        rope = dict(positions=positions, cos_sin=self.cos_sin, slots=slot_mapping, q_out=self.buf_q, k_cache=kc, v_cache=vc,
                    nh=self.nh, nkv=self.nkv, hd=self.hd, block_size=self.block_size)
        res, xf = self.buf_res, self.buf_xf
        wq, bias = w[p + "self_attn.qkv_proj.weight"], w.get(p + "self_attn.qkv_proj.bias")
        if src is _PLAN:
            src = self._plan_src("d", T) if li > 0 else None
        # residual is None on layer 0 (llama3.py:187-190): residual := embeddings, x := norm(embeddings)
        res_in = None if li == 0 else res
        if norm_fuse:
            H.gemm_fused(wq, T, self.qkv_n, self.h, H.FEPI_QKV_ROPE, res_in=res_in, res_out=self.buf_res2, norm_w=w[p + "input_layernorm.weight"],
                         eps=cfg.rms_norm_eps, bias=bias, waves=16, **self._prologue_src(src), **rope)
            return
        if not gemm_only:
            self._add_norm(src, T, w[p + "input_layernorm.weight"], res_in=res_in, res_out=res, out_frag=xf)
        if small or (16 < T <= 32 and not cfg.qk_norm and not self.quantized and not self.kv8 and not lora):      # T in 17..32 (tree-decode step): the two-token-tile variant
            H.gemm_fused(wq, T, self.qkv_n, self.h, H.FEPI_QKV_ROPE, x_frag=xf, bias=bias, **rope)
            return
        head_norm = dict(q_norm_w=w.get(p + "self_attn.q_norm.weight"), k_norm_w=w.get(p + "self_attn.k_norm.weight"), eps=cfg.rms_norm_eps,
                         qkv_perm=1)
        if not gemm_only and not self.kv8 and not lora and bias is None and self._pf_partials_ok(T, self.qkv_n, self.h):
            # single-chunk prefill of a big QKV matrix: its split-K slabs stay in the workspace and the RoPE / KV-store kernel
            # sums them (bit-identical to the GEMM's epilogue launch + rope_store_kv; one launch less per layer)
            qkv = self._gemm_pf_partials(xf, self.h, wq, self.qkv_n, T, min_splits=2)
            if qkv is not None:
                H.rope_store_kv_parts(qkv.buf, qkv.n, positions, self.cos_sin, slot_mapping, self.buf_q, kc, vc, T, self.nh, self.nkv,
                                      self.hd, self.block_size, **head_norm)
                return
        self._gemm(xf, self.h, p + "self_attn.qkv_proj.weight", self.qkv_n, self.buf_qkv, T, self.qkv_n, bias=bias)
        if gemm_only:
            return
        if lora:
            self._lora_delta(li, "qkv", xf, self.buf_qkv, T, self.qkv_n)
        if self.kv8:
            KV8.rope_store_kv_fp8(self.buf_qkv, positions, self.cos_sin, slot_mapping, self.buf_q, kc, vc, T, self.nh, self.nkv,
                                  self.hd, self.block_size, k_inv_scale=self.kv_inv_scale[li, 0], v_inv_scale=self.kv_inv_scale[li, 1],
                                  **head_norm)
            return
        H.rope_store_kv(self.buf_qkv, positions, self.cos_sin, slot_mapping, self.buf_q, kc, vc, T, self.nh, self.nkv,
                        self.hd, self.block_size, **head_norm)

    def _launch_to_h(self, which: str, li: int, T: int, parts: bool | None, pf_partials: bool) -> Slabs | None:
        """o_proj ("o") / down_proj ("d"): the [h, K] GEMM whose result the next norm reads.  Returns the hand-off: the prefill GEMM's
        split-K slabs in the workspace (pf_partials, one prefill chunk of a big matrix), ssd_gemm_parts' slabs (parts; None: as
        parts_plan says), or None for rows in buf_h."""
        name, xf, K, slabs = ((f"model.layers.{li}.self_attn.o_proj.weight", self.buf_af, self.qn, self.buf_parts_o) if which == "o" else
                              (f"model.layers.{li}.mlp.down_proj.weight", self.buf_actf, self.I, self.buf_parts_d))
        if which == "d" and self.moe:
            self._moe_down(li, T)
            return None
        w = self.w[name]
        if self.lora_active:        # rows into buf_h, then the delta: no slabs of any kind
            self._gemm(xf, K, name, self.h, self.buf_h, T, self.h)
            self._lora_delta(li, "o" if which == "o" else "down", xf, self.buf_h, T, self.h)
            return None
        if pf_partials and self._pf_partials_ok(T, self.h, K):
            return self._gemm_pf_partials(xf, K, w, self.h, T)
        if self.parts_plan(T) if parts is None else parts:
            S, wv = self._parts(which, T)
            H.gemm_parts(xf, w, T, self.h, K, parts=slabs, splits=S, waves=wv)
            return Slabs(slabs, S, T)
        self._gemm(xf, K, name, self.h, self.buf_h, T, self.h)
        return None

    def launch_o(self, li: int, T: int, parts: bool | None = None, pf_partials: bool = False) -> Slabs | None:
        return self._launch_to_h("o", li, T, parts, pf_partials)

    def launch_gate_up(self, li: int, T: int, gemm_only: bool = False, src=_PLAN) -> None:
        """src: the hand-off of o_proj (the split-K GEMM leaves its own number of slabs, the fused attention + o_proj nkv)."""
        cfg, w = self.cfg, self.w
        p = f"model.layers.{li}."
        if src is _PLAN:
            src = self._plan_src("o", T)
        if self.moe:
            if not gemm_only:
                self._add_norm(src, T, w[p + "post_attention_layernorm.weight"], res_in=self.buf_res, res_out=self.buf_res,
                               out_rows=self.moe_x, out_frag=self.buf_xf)
            self._moe_up(li, T)
            return
        if self.lora_active:        # rows in the packed gate / up order -> delta -> SiLU * mul of the updated rows, fragment-major
            if not gemm_only:
                self._add_norm(src, T, w[p + "post_attention_layernorm.weight"], res_in=self.buf_res, res_out=self.buf_res, out_frag=self.buf_xf)
            self._gemm(self.buf_xf, self.h, p + "mlp.gate_up_proj.weight", 2 * self.I, self.buf_gu, T, 2 * self.I, epi=H.EPI_ROWS)
            self._lora_delta(li, "gate_up", self.buf_xf, self.buf_gu, T, 2 * self.I, act_frag=self.buf_actf)
            return
        if self.fusion_plan(T)[1]:
            H.gemm_fused(w[p + "mlp.gate_up_proj.weight"], T, 2 * self.I, self.h, H.FEPI_SILU_FRAG,
                         res_in=self.buf_res2, res_out=self.buf_res, norm_w=w[p + "post_attention_layernorm.weight"],
                         eps=cfg.rms_norm_eps, y=self.buf_actf, waves=8, **self._prologue_src(src))     # profiles/micro/fused_probe.py: 13.2 us vs 16.4 (16 waves)
            return
        if not gemm_only:
            self._add_norm(src, T, w[p + "post_attention_layernorm.weight"], res_in=self.buf_res, res_out=self.buf_res, out_frag=self.buf_xf)
        self._gemm(self.buf_xf, self.h, p + "mlp.gate_up_proj.weight", 2 * self.I, self.buf_actf, T, 0, epi=H.EPI_SILU_FRAG)

    def launch_down(self, li: int, T: int, parts: bool | None = None, pf_partials: bool = False) -> Slabs | None:
        return self._launch_to_h("d", li, T, parts, pf_partials)

    def forward(self, input_ids: torch.Tensor, positions: torch.Tensor, T: int, meta: AttnMeta) -> None:
        """Runs all layers; leaves the final (pre-norm) hidden state in buf_h and the residual in buf_res."""
        cfg, w = self.cfg, self.w
        h = self.buf_h
        H.embedding(input_ids, w["model.embed_tokens.weight"], h, T, self.h,
                    vocab_start=self.tp_rank * self.V if self.tp_size > 1 else 0, vocab_count=self.V if self.tp_size > 1 else cfg.vocab_size)
        self._allreduce(h[:T])
        splits, attn_waves = self._attn_cfg(T, meta)
        attn_flags = self._attn_flags(meta)
        scale = self.hd ** -0.5
        # compute_logits, which always follows in the same Python body, reads the last hand-off: the segments leave rows (buf_h) + the
        # residual (buf_res)
        self._last = None
        lora = self.lora_active
        assert not lora or (self.max_loras and meta.mode == H.MODE_CAUSAL), "an adapted forward needs the slot tables and causal rows"
        if not lora and self.chain_plan(T, meta, splits):
            self._forward_chain(positions, meta, attn_waves)
            return
        if not lora and self.tree_plan(T, meta):
            self._forward_tree_seg(positions, T, meta, splits, attn_waves)
            return
        # a varlen prefill never takes the slab path (its last-token gather reads rows)
        parts = self.parts_plan(T) and meta.cu_q is None and not lora
        fuse_ao = parts and self.attn_o_plan(T, meta, splits)
        # tensor parallel with the one-shot collective: the all-reduce after o_proj / down_proj absorbs the residual add
        # and the RMSNorm that follow it (csrc/comm.hip), 2 launches fewer per half layer
        ar = self.custom_ar
        fuse = self.use_coll and ar is not None and self.fuse_ar_norm and ar.fits_rows(T, self.h)
        eps, res, xf = cfg.rms_norm_eps, self.buf_res, self.buf_xf
        L = cfg.num_layers
        src = None          # the hand-off: the embedding is rows in buf_h
        for li in range(L):
            self.launch_qkv(li, T, positions, meta.slot_mapping, src=src)
            if self.taps is not None and li in self.taps:
                # launch_qkv has just written x + residual: to buf_res2 on the fused-prologue path, to buf_res otherwise
                tap = self.buf_res2 if self.fusion_plan(T)[1] else res
                i = self.taps.index(li)
                self.acts[:T, i * self.h:(i + 1) * self.h].copy_(tap[:T])
            if fuse_ao:
                H.attn_oproj_parts(self.buf_q, self.kv_cache[li, 0], self.kv_cache[li, 1], meta.block_tables, self.max_blocks,
                                   meta.context_lens, T, self.nh, self.nkv, self.hd, self.block_size, scale,
                                   w[f"model.layers.{li}.self_attn.o_proj.weight"], self.h, self.buf_parts_o)
                src = Slabs(self.buf_parts_o, self.nkv, T)
            else:
                self._attn(li, T, meta, splits, attn_flags, attn_waves, scale)
                src = self.launch_o(li, T, parts=parts, pf_partials=not parts)
            if fuse:
                ar.all_reduce_add_rmsnorm(h, res, res, w[f"model.layers.{li}.post_attention_layernorm.weight"], eps, T, self.h, out_frag=xf)
                src = NORMED
            else:
                self._allreduce(h[:T])
            self.launch_gate_up(li, T, src=src)
            # (the last layer's down_proj keeps its epilogue: compute_logits' last-token gather reads rows)
            src = self.launch_down(li, T, parts=parts, pf_partials=not parts and li + 1 < L)
            if fuse and li + 1 < L:
                ar.all_reduce_add_rmsnorm(h, res, res, w[f"model.layers.{li + 1}.input_layernorm.weight"], eps, T, self.h, out_frag=xf)
                src = NORMED
            else:
                self._allreduce(h[:T])
        self._last = src


    def compute_logits(self, T: int, gather: torch.Tensor | None = None, rows: int | None = None) -> int:
        """Final add+RMSNorm (optionally only the `gather` rows: prefill last-token, embed_head.py:81-84) and the
        LM-head GEMM into self.logits[:rows] (this rank's vocab shard).  Returns the number of logit rows."""
        n = T if gather is None else rows
        assert n <= self.max_logit_rows
        self._add_norm(self._last, n, self.w["model.norm.weight"], res_in=self.buf_res, out_frag=self.buf_lastf, gather=gather)
        if self._ap_ok(n):
            H.gemm_argmax(self.buf_lastf, self.w["lm_head.weight"], self.logits, n, self.V, self.h, self.V, self.ap_val, self.ap_idx,
                          self.ap_stride)
        else:
            self._gemm(self.buf_lastf, self.h, self.w["lm_head.weight"], self.V, self.logits, n, self.V)
        return n

    def compute_logits_into(self, gather: torch.Tensor, n: int, frag: torch.Tensor, out: torch.Tensor) -> None:
        """The same for the n rows `gather` names of the forward that has just run, into the caller's buffers: norm output fragment
        `frag`, logits `out` [n][V] (the prompt log-probability pass walks a prefill's rows in chunks).  The final norm can be run again
        and again: a varlen prefill hands over rows (buf_h), and the norm only reads them and the residual."""
        assert self._last is None and self.tp_size == 1, "the prompt pass needs the row hand-off of a single-rank prefill"
        self._add_norm(None, n, self.w["model.norm.weight"], res_in=self.buf_res, out_frag=frag, gather=gather)
        self._gemm(frag, self.h, self.w["lm_head.weight"], self.V, out, n, self.V)

    def _ap_ok(self, n: int) -> bool:
        """compute_logits(n) leaves argmax candidates for its n rows."""
        return self.argmax_fused and n <= self.ap_rows

    def _ap_parts(self, n: int) -> int:
        return H.gemm_argmax_nparts(n, self.V, self.h)

    def has_argmax_parts(self, n: int) -> bool:
        """compute_logits(n) leaves argmax candidates and the vocabulary is not sharded (the fused tails apply)."""
        return self._ap_ok(n) and not self.use_coll

    def argmax_verify(self, B: int, K: int, speculations, preds, accept_len, recovery, packed) -> None:
        """argmax of the B*(K+1) verify rows + greedy accept / reject (utils/verify.py:28-48) in one launch (TP = 1)."""
        assert self.has_argmax_parts(B * (K + 1))
        H.argmax_parts_verify(self.ap_val, self.ap_idx, self._ap_parts(B * (K + 1)), self.ap_stride, speculations, B, K, accept_len, recovery,
                              packed, preds=preds)

    def argmax_advance(self, B: int, next_ids, input_ids, positions, slots, context_lens, block_tables, max_blocks, block_size,
                       spec, K, step) -> None:
        """argmax of the B decode rows + the device-side chain advance (csrc/misc.hip draft_advance) in one launch."""
        assert self.has_argmax_parts(B)
        H.argmax_parts_advance(self.ap_val, self.ap_idx, self._ap_parts(B), self.ap_stride, next_ids, input_ids, positions, slots,
                               context_lens, block_tables, max_blocks, block_size, spec, K, step, B)

    def argmax(self, n: int, out: torch.Tensor, out2: torch.Tensor | None = None, out3: torch.Tensor | None = None,
               out3_stride: int = 0) -> None:
        """Greedy tokens of logits[:n] over the FULL vocabulary (identical on every TP rank).  out3 (optional): a third
        destination written with a row stride (the tree step's [T][K] token table; only with candidates available)."""
        if not self.use_coll:
            if self._ap_ok(n):          # candidates from the LM-head epilogue: a few thousand per row instead of V logits
                H.argmax_parts(self.ap_val, self.ap_idx, self._ap_parts(n), self.ap_stride, n, out, out2, out3, out3_stride)
            else:
                assert out3 is None
                H.argmax_rows(self.logits, self.V, n, self.V, out, out2)
            return
        assert out3 is None
        R = self.max_logit_rows
        # one-shot exchange: local (global index, value) straight into this rank's packed buffer; else the two gather sources
        packed = self.custom_ar is not None
        idx_l, val_l = (self.am_pack_l[:R], self.am_pack_l[R:].view(torch.float32)[:R]) if packed else (self.am_idx_l, self.am_val_l)
        self._argmax_local(n, idx_l, val_l)
        self._argmax_merge(n, out, out2, packed)

    def _argmax_local(self, n: int, idx_l, val_l) -> None:
        """This rank's best (global index, value) per row of logits[:n]: from the LM-head candidates, else from the logits."""
        if self._ap_ok(n):
            H.argmax_parts(self.ap_val, self.ap_idx, self._ap_parts(n), self.ap_stride, n, idx_l, out_val=val_l, idx_offset=self.tp_rank * self.V)
        else:
            H.argmax_rows_val(self.logits, self.V, n, self.V, self.tp_rank * self.V, idx_l, val_l)

    def _argmax_merge(self, n: int, out, out2, packed: bool) -> None:
        """Every rank's local best -> the winner per row, on every rank: one one-shot all-gather of the packed buffers (rank r's indices
        start at word r * am_words, its values R words later: one strided merge), or two torch.distributed all-gathers into [tp][R]
        (rows beyond n are ignored by the merge: T = n, stride R)."""
        R = self.max_logit_rows
        if packed:
            self.custom_ar.all_gather_words(self.am_pack_l, self.am_pack, self.am_words)
            vals = self.am_pack.view(-1)[R:].view(torch.float32)
            H.argmax_merge(vals, self.am_pack, self.tp_size, n, 2 * self.am_words, out, out2, stride_idx=self.am_words)
            return
        dist.all_gather_into_tensor(self.am_val.view(-1), self.am_val_l, group=self.tp_group)
        dist.all_gather_into_tensor(self.am_idx.view(-1), self.am_idx_l, group=self.tp_group)
        H.argmax_merge(self.am_val, self.am_idx, self.tp_size, n, R, out, out2)

    def full_logits(self, n: int) -> torch.Tensor:
        """[n, V_full] logits on every rank (only needed off the greedy path)."""
        if not self.use_coll:
            return self.logits[:n]
        parts = [torch.empty(n, self.V, dtype=BF16, device=self.device) for _ in range(self.tp_size)]
        dist.all_gather(parts, self.logits[:n].contiguous(), group=self.tp_group)
        return torch.cat(parts, dim=-1)
