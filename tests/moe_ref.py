"""float64 restatement of the mixture-of-experts semantics of include/ssd_hip_moe.h and of a whole Qwen3-MoE forward, shared by
tests/test_moe_cpu.py, tests/test_hip_moe.py and tests/test_moe_engine_gpu.py.

The three kernels (entry p = t * k + j is choice j of token row t):
    route    ids = the k largest logits, larger first, ties to the lower index; w = bf16(softmax(l)[ids] / (norm ? their sum : 1));
             offs / perm = the entries grouped by expert, ascending entry index inside an expert
    gemm     up:   act[p] = bf16(silu(g) * u), g = bf16(x[t] . Wg[e]^T), u = bf16(x[t] . Wu[e]^T)
             down: d[p]   = bf16(act[p] . Wd[e]^T)
    combine  h[t] = bf16(sum_j w[t][j] * float(d[t k + j])), j ascending, fp32 products and sums
Everything but combine_ref is computed in float64 from the bf16 inputs: the exact value the kernels' roundings are measured against.

forward() is the model: float64 "truth" (nothing rounded) or, with pipeline=True, the same arithmetic rounded to bf16 at the points
where the engine stores bf16.  Both take forced_routes: per layer the topk_ids [T, k] that replace the forward's own choice, the
routing weights still computed from the forward's own logits at those ids.
"""
import torch

from tests.lora_ref import assert_within_bar, bf16_ulp  # noqa: F401  (the GEMM bar, re-exported)

F64 = torch.float64
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def topk_ids(logits: torch.Tensor, k: int) -> torch.Tensor:
    """[T, E] -> int64 [T, k]: the k largest, larger first, ties to the lower expert index (a stable sort of the negated values)."""
    return torch.sort(-logits.to(F64), dim=-1, stable=True).indices[:, :k]


def route_weights(logits: torch.Tensor, ids: torch.Tensor, norm: bool, rnd=None, softmax_dtype=F64) -> torch.Tensor:
    """float64 softmax over all E logits at `ids`, divided by their sum when norm; rnd (optional) rounds the result.  softmax_dtype
    float32: the softmax and the division as transformers' router does them (forward(hf_float32_points=True))."""
    w = torch.softmax(logits.to(F64), dim=-1, dtype=softmax_dtype).gather(1, ids.long())
    if norm:
        w = w / w.sum(-1, keepdim=True)
    w = w.to(F64)
    return w if rnd is None else rnd(w)


def group_tables(ids: torch.Tensor, E: int):
    """ids [T, k] -> (offs int32 [E + 1], perm int32 [T k]): the entries grouped by expert, ascending entry index inside an expert."""
    flat = ids.reshape(-1).long()
    perm = torch.sort(flat, stable=True).indices
    offs = torch.zeros(E + 1, dtype=torch.long, device=ids.device)
    offs[1:] = torch.bincount(flat, minlength=E).cumsum(0)
    return offs.int(), perm.int()


def route_ref(logits: torch.Tensor, k: int, norm: bool):
    """-> (ids int32 [T, k], w bf16 [T, k], offs, perm) of bf16 / float router-logit rows [T, E]."""
    ids = topk_ids(logits, k)
    w = route_weights(logits, ids, norm).to(BF)
    offs, perm = group_tables(ids, logits.shape[-1])
    return ids.int(), w, offs, perm


def grouped_exact(rows: torch.Tensor, W: torch.Tensor, ids: torch.Tensor, gather_tokens: bool):
    """rows [T, K] (gather_tokens: entry p reads row p // k) or [T k, K]; W [E, N, K]; ids [T, k] -> (y float64 [T k, N], mag): every
    entry's row times its expert's matrix, and sum |x w|.  One expert at a time (only the chosen ones)."""
    T, k = ids.shape
    flat = ids.reshape(-1).long()
    src = torch.arange(T * k, device=rows.device) // k if gather_tokens else torch.arange(T * k, device=rows.device)
    y = torch.zeros(T * k, W.shape[1], dtype=F64, device=rows.device)
    mag = torch.zeros_like(y)
    for e in flat.unique().tolist():
        sel = (flat == e).nonzero().squeeze(1)
        x = rows[src[sel]].to(F64)
        We = W[e].to(F64)
        y[sel] = x @ We.t()
        mag[sel] = x.abs() @ We.abs().t()
    return y, mag


def silu_mul_bf16(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """float64 silu(g) * u of bf16-representable g, u (not rounded)."""
    g, u = g.to(F64), u.to(F64)
    return g / (1.0 + torch.exp(-g)) * u


def bf16_neighbours(b: torch.Tensor):
    """A bf16 tensor -> (itself, the next bf16 value towards zero, the next away from zero): the bit pattern -1 / +1."""
    bits = b.contiguous().view(torch.int16)
    return b, (bits - 1).view(BF), (bits + 1).view(BF)


def assert_act_within_bar(act: torch.Tensor, g64, gmag, u64, umag, what: str = "") -> None:
    """act = bf16(silu(gb) * ub) where gb, ub are g, u as the GEMM rounded them.  The GEMM bar (1 bf16 ulp of the float64 value,
    differences below 2^-20 * sum|x w| exempt) is a bar on gb and ub, not on their product through silu (one ulp of g moves silu(g) * u
    by about an ulp, which the final rounding can turn into two).  So: act must be within 1 bf16 ulp of silu(gb') * ub' for SOME
    (gb', ub') among bf16(g64), bf16(u64) and their two bf16 neighbours that themselves meet the GEMM bar; the bar's exemption is
    carried through the product by its derivatives: |d act| <= 1.1 |u| dg + |silu(g)| du with dg = 2^-20 sum|x wg|, du likewise
    (|silu'| <= 1.1)."""
    got = act.to(F64)
    ok = torch.zeros_like(got, dtype=torch.bool)

    def cands(v64, mag):
        bar = torch.maximum(bf16_ulp(v64), mag * 2.0 ** -20)
        return [(c.to(F64), (c.to(F64) - v64).abs() <= bar) for c in bf16_neighbours(v64.to(BF))]

    for gb, g_ok in cands(g64, gmag):
        for ub, u_ok in cands(u64, umag):
            want = silu_mul_bf16(gb, ub)
            floor = (1.1 * ub.abs() * gmag + (want / ub.abs().clamp(min=1e-300)).abs() * umag) * 2.0 ** -20
            ok |= g_ok & u_ok & ((got - want).abs() <= torch.maximum(bf16_ulp(want), floor))
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} activations outside the bar"


def combine_ref(d: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """d bf16 [T k, H], w fp32 [T, k] -> bf16 [T, H]: the kernel's own arithmetic (fp32 product, fp32 sum, j ascending, one rounding)."""
    T, k = w.shape
    dd = d.view(T, k, -1).float()
    acc = torch.zeros(T, dd.shape[-1], dtype=torch.float32, device=d.device)
    for j in range(k):
        acc = acc + w[:, j, None].float() * dd[:, j]
    return acc.to(BF)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def forward(cfg, w: dict, tokens, pipeline: bool = False, forced_routes=None, hf_float32_points: bool = False):
    """Qwen3-MoE over one full sequence with causal attention (mathematically equal to prefill + cached decode / verify).
    -> (logits float64 [T, V], router logits per layer float64 [T, E], topk ids per layer int64 [T, k]).
    pipeline=False: float64, nothing rounded.  pipeline=True: every value the engine stores as bf16 is rounded to bf16 there (the
    residual, the norm outputs, every GEMM output, q / k after the head norm and RoPE, the attention output, the router logits, the
    routing weights, g, u, act, d, the combined h, the logits); between two roundings the arithmetic stays float64.
    hf_float32_points: the three computations transformers' modules do in float32 whatever the model's dtype -- the rotary table
    (Qwen3MoeRotaryEmbedding.forward: inv_freq.float() @ positions.float(), cos / sin of that), every RMSNorm's normalisation
    (Qwen3MoeRMSNorm.forward: hidden_states.to(torch.float32)) and the router's softmax (Qwen3MoeTopKRouter.forward:
    softmax(..., dtype=torch.float)) -- are done in float32 here too, so that a "float64" Qwen3MoeForCausalLM can be matched to
    1e-9; the truth proper (False) has no such point and differs from that model by a few float32 roundings (~1e-6 relative)."""
    D = F64
    rnd = (lambda x: x.to(BF).to(D)) if pipeline else (lambda x: x)
    T = len(tokens)
    hd, nh, nkv = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    E, k = cfg.num_experts, cfg.num_experts_per_tok
    h = w["model.embed_tokens.weight"].to(D)[torch.tensor(list(tokens))]
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=D) / hd))
    fr = torch.arange(T, dtype=D)[:, None] * inv[None, :]
    if pipeline or hf_float32_points:       # the engine's table is fp32 (model.make_cos_sin), and so is transformers' 
        inv32 = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))
        fr32 = torch.einsum("i,j -> ij", torch.arange(T, dtype=torch.float), inv32)
        cos, sin = fr32.cos().to(D)[:, None, :], fr32.sin().to(D)[:, None, :]
    else:
        cos, sin = fr.cos()[:, None, :], fr.sin()[:, None, :]

    def norm(x, wt):
        if hf_float32_points:       # Qwen3MoeRMSNorm.forward: the normalisation in float32, the weight applied in the model's dtype
            x32 = x.to(torch.float32)
            x32 = x32 * torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + cfg.rms_norm_eps)
            return wt.to(D) * x32.to(D)
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.rms_norm_eps) * wt.to(D)

    def rot(x):
        x1, x2 = x.chunk(2, -1)
        return torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1)

    mask = torch.full((T, T), float("-inf"), dtype=D).triu(1)
    res = None
    all_logits, all_ids = [], []
    for li in range(cfg.num_layers):
        p = f"model.layers.{li}."
        s = h if res is None else h + res
        res = rnd(s)
        x = rnd(norm(s, w[p + "input_layernorm.weight"]))
        qkv = rnd(x @ w[p + "self_attn.qkv_proj.weight"].to(D).t())
        q, kk, v = qkv.split([nh * hd, nkv * hd, nkv * hd], -1)
        q, kk, v = q.view(T, nh, hd), kk.view(T, nkv, hd), v.view(T, nkv, hd)
        q = rnd(rot(norm(q, w[p + "self_attn.q_norm.weight"])))
        kk = rnd(rot(norm(kk, w[p + "self_attn.k_norm.weight"])))
        g = nh // nkv
        kk, v = kk.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
        sc = torch.einsum("qhd,khd->hqk", q, kk) * hd ** -0.5 + mask
        o = rnd(torch.einsum("hqk,khd->qhd", sc.softmax(-1), v).reshape(T, nh * hd))
        h = rnd(o @ w[p + "self_attn.o_proj.weight"].to(D).t())
        s = h + res
        res = rnd(s)
        x = rnd(norm(s, w[p + "post_attention_layernorm.weight"]))
        # ---- the sparse block ----
        rl = rnd(x @ w[p + "mlp.gate.weight"].to(D).t())
        ids = topk_ids(rl, k) if forced_routes is None else forced_routes[li].long()
        rw = route_weights(rl, ids, cfg.norm_topk_prob, rnd, softmax_dtype=torch.float32 if hf_float32_points else F64)
        all_logits.append(rl)
        all_ids.append(ids)
        gu, _ = grouped_exact(x, w[p + "mlp.experts.gate_up_proj"], ids, gather_tokens=True)
        gu = rnd(gu)
        ga, up = gu.chunk(2, -1)
        act = rnd(ga / (1.0 + torch.exp(-ga)) * up)
        d, _ = grouped_exact(act, w[p + "mlp.experts.down_proj"], ids, gather_tokens=False)
        d = rnd(d).view(T, k, -1)
        h = rnd((rw[:, :, None] * d).sum(1))
    x = rnd(norm(h + res, w["model.norm.weight"]))
    head = w["model.embed_tokens.weight"] if cfg.tie_word_embeddings else w["lm_head.weight"]
    return rnd(x @ head.to(D).t()), all_logits, all_ids


def kth_margins(router_logits: torch.Tensor, k: int) -> torch.Tensor:
    """[T, E] -> [T]: the k-th largest logit minus the (k+1)-th, and [T] the k-th value (the larger of the two)."""
    top = torch.sort(router_logits.to(F64), dim=-1, descending=True).values
    return top[:, k - 1] - top[:, k], top[:, k - 1]


def tiny_moe_config(**kw):
    """The configuration the CPU and engine tests share: 2 layers, h 128, 4 heads, 2 kv heads, head_dim 32, 8 experts, top 2,
    moe_intermediate 64, vocab 512."""
    from ssd_amd.model_config import ModelConfig
    base = dict(family="qwen3_moe", hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=32, intermediate_size=64,
                vocab_size=512, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=1024, tie_word_embeddings=False, qk_norm=True,
                num_experts=8, num_experts_per_tok=2, moe_intermediate_size=64, norm_topk_prob=True)
    base.update(kw)
    return ModelConfig(**base)
