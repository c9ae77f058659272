"""Float64 reference of a sliding-window model: tests/util.truth_forward with a visibility matrix per layer.  Layer li with window
W = cfg.window_of(li) lets query i see the keys j with i - W < j <= i (W = 0: every j <= i).  Nothing is rounded in between; with one
window for every layer it is truth_forward_masked under that mask (tests/test_swa_cpu.py holds the two together)."""
import torch

D = torch.float64


def visible(T: int, W: int) -> torch.Tensor:
    i, j = torch.arange(T).view(-1, 1), torch.arange(T).view(1, -1)
    return (j <= i) & ((j > i - W) if W else (j <= i))


def forward(cfg, w: dict, tokens: list[int]) -> torch.Tensor:
    T = len(tokens)
    hd, nh, nkv = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    fr = torch.arange(T, dtype=D)[:, None] / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=D) / hd))[None, :]
    cos, sin = fr.cos()[:, None, :], fr.sin()[:, None, :]

    def norm(x, wt):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.rms_norm_eps) * wt.to(D)

    def rot(x):
        x1, x2 = x.chunk(2, -1)
        return torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1)

    res = w["model.embed_tokens.weight"].to(D)[torch.tensor(tokens)]
    for li in range(cfg.num_layers):
        p = f"model.layers.{li}."
        qkv = norm(res, w[p + "input_layernorm.weight"]) @ w[p + "self_attn.qkv_proj.weight"].to(D).t()
        q, k, v = (t.view(T, -1, hd) for t in qkv.split([nh * hd, nkv * hd, nkv * hd], -1))
        if cfg.qk_norm:
            q, k = norm(q, w[p + "self_attn.q_norm.weight"]), norm(k, w[p + "self_attn.k_norm.weight"])
        q, k, v = rot(q), rot(k).repeat_interleave(nh // nkv, 1), v.repeat_interleave(nh // nkv, 1)
        s = (torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5).masked_fill(~visible(T, cfg.window_of(li)), float("-inf"))
        res = res + torch.einsum("hqk,khd->qhd", s.softmax(-1), v).reshape(T, nh * hd) @ w[p + "self_attn.o_proj.weight"].to(D).t()
        a, b = (norm(res, w[p + "post_attention_layernorm.weight"]) @ w[p + "mlp.gate_up_proj.weight"].to(D).t()).chunk(2, -1)
        res = res + (a * torch.sigmoid(a) * b) @ w[p + "mlp.down_proj.weight"].to(D).t()
    head = w["model.embed_tokens.weight"] if cfg.tie_word_embeddings else w["lm_head.weight"]
    return norm(res, w["model.norm.weight"]) @ head.to(D).t()
