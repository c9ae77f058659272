"""Torch restatement of the FP8 KV cache format (include/ssd_hip_kv8.h) for the tests, written from its definition and independent
of ssd_amd/quant.py, plus the two references an fp8-KV target is held against: the CPU oracle model and the float64 truth, each with
k and v replaced by decode(encode(.)) of their bf16 rounding -- what the HIP target reads back from its cache."""
from __future__ import annotations

import torch

from oracle.model import OracleModel

BF = torch.bfloat16


def _table() -> torch.Tensor:
    """The 256 e4m3fn values from the bit fields: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is subnormal
    (m / 8 * 2^-6); 0x7F and 0xFF are NaN; there is no infinity."""
    out = []
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        out.append(-v if s else v)
    return torch.tensor(out, dtype=torch.float32)


TABLE = _table()
FINITE_CODES = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=torch.uint8)


def encode(x_bf16: torch.Tensor, inv_scale) -> torch.Tensor:
    """code = e4m3fn_rne(clamp(fp32(x) * inv_scale, -448, 448)); torch's cast rounds to nearest even and keeps -0.0 but does not
    saturate, so the clamp comes first."""
    assert x_bf16.dtype == BF
    inv = torch.as_tensor(inv_scale, dtype=torch.float32, device=x_bf16.device)
    return torch.clamp(x_bf16.float() * inv, -448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def decode(codes: torch.Tensor, scale) -> torch.Tensor:
    """fp32 scale * value(code), the value looked up in the bit-field table."""
    assert codes.dtype == torch.uint8
    s = torch.as_tensor(scale, dtype=torch.float32, device=codes.device)
    return s * TABLE.to(codes.device)[codes.long()]


def roundtrip(x_bf16: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x [T, nkv, hd] bf16, scale fp32 [nkv] -> bf16(decode(encode(x))) with the host's fp32 inverse."""
    s = scale.float().view(-1, 1)
    return decode(encode(x_bf16, 1.0 / s), s).to(BF)


class Kv8OracleModel(OracleModel):
    """OracleModel whose attention sees k and v as an fp8 KV cache returns them: both are replaced by decode(encode(.)) before they
    are stored or attended over -- in the prefill branch that attends over the fresh k / v as well, because the HIP prefill reads
    back what it stored.  k_scale / v_scale: fp32 [L, nkv] (default all 1.0)."""

    def set_kv_scales(self, k_scale=None, v_scale=None):
        L = self.cfg.num_layers
        self.k_scale = torch.ones(L, self.nkv) if k_scale is None else torch.as_tensor(k_scale, dtype=torch.float32).reshape(L, self.nkv)
        self.v_scale = torch.ones(L, self.nkv) if v_scale is None else torch.as_tensor(v_scale, dtype=torch.float32).reshape(L, self.nkv)

    def _attention(self, li: int, q, k, v, ctx):
        if not hasattr(self, "k_scale"):
            self.set_kv_scales()
        T, hd = q.shape[0], self.cfg.head_dim
        k = roundtrip(k.reshape(T, self.nkv, hd).to(BF), self.k_scale[li]).to(k.dtype).reshape(k.shape)
        v = roundtrip(v.reshape(T, self.nkv, hd).to(BF), self.v_scale[li]).to(v.dtype).reshape(v.shape)
        return OracleModel._attention(self, li, q, k, v, ctx)


def as_kv8_oracle(model: OracleModel, k_scale=None, v_scale=None) -> OracleModel:
    """Turn an existing OracleModel INSTANCE (an oracle engine's target runner's model) into a Kv8OracleModel in place."""
    assert type(model) is OracleModel, type(model)
    model.__class__ = Kv8OracleModel
    model.set_kv_scales(k_scale, v_scale)
    return model


def truth_forward_kv8(cfg, w: dict, tokens: list[int], k_scale=None, v_scale=None) -> torch.Tensor:
    """tests/util.truth_forward (float64, nothing else rounded) with rot(k) and v replaced by decode(encode(.)) of their bf16
    rounding: the exact arithmetic over what an fp8 KV cache holds."""
    D = torch.float64
    T = len(tokens)
    L = cfg.num_layers
    h = w["model.embed_tokens.weight"].to(D)[torch.tensor(tokens)]
    hd, nh, nkv = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    ks = torch.ones(L, nkv) if k_scale is None else torch.as_tensor(k_scale, dtype=torch.float32).reshape(L, nkv)
    vs = torch.ones(L, nkv) if v_scale is None else torch.as_tensor(v_scale, dtype=torch.float32).reshape(L, nkv)
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=D) / hd))
    fr = torch.arange(T, dtype=D)[:, None] * inv[None, :]
    cos, sin = fr.cos()[:, None, :], fr.sin()[:, None, :]

    def norm(x, wt, eps):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * wt.to(D)

    def rot(x):
        x1, x2 = x.chunk(2, -1)
        return torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1)

    mask = torch.full((T, T), float("-inf"), dtype=D).triu(1)
    res = None
    for li in range(L):
        p = f"model.layers.{li}."
        res = h if res is None else h + res
        x = norm(res, w[p + "input_layernorm.weight"], cfg.rms_norm_eps)
        qkv = x @ w[p + "self_attn.qkv_proj.weight"].to(D).t()
        if p + "self_attn.qkv_proj.bias" in w:
            qkv = qkv + w[p + "self_attn.qkv_proj.bias"].to(D)
        q, k, v = qkv.split([nh * hd, nkv * hd, nkv * hd], -1)
        q, k, v = q.view(T, nh, hd), k.view(T, nkv, hd), v.view(T, nkv, hd)
        if cfg.qk_norm:
            q = norm(q, w[p + "self_attn.q_norm.weight"], cfg.rms_norm_eps)
            k = norm(k, w[p + "self_attn.k_norm.weight"], cfg.rms_norm_eps)
        q, k = rot(q), rot(k)
        k = decode(encode(k.to(BF), 1.0 / ks[li].view(-1, 1)), ks[li].view(-1, 1)).to(D)
        v = decode(encode(v.to(BF), 1.0 / vs[li].view(-1, 1)), vs[li].view(-1, 1)).to(D)
        g = nh // nkv
        k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
        s = torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5 + mask
        o = torch.einsum("hqk,khd->qhd", s.softmax(-1), v).reshape(T, nh * hd)
        h = o @ w[p + "self_attn.o_proj.weight"].to(D).t()
        res = h + res
        x = norm(res, w[p + "post_attention_layernorm.weight"], cfg.rms_norm_eps)
        gu = x @ w[p + "mlp.gate_up_proj.weight"].to(D).t()
        a, b = gu.chunk(2, -1)
        h = (a * torch.sigmoid(a) * b) @ w[p + "mlp.down_proj.weight"].to(D).t()
    x = norm(h + res, w["model.norm.weight"], cfg.rms_norm_eps)
    head = w["model.embed_tokens.weight"] if cfg.tie_word_embeddings else w["lm_head.weight"]
    return x @ head.to(D).t()
