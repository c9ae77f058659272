"""FP8 KV cache (kv_cache_dtype="fp8", include/ssd_hip_kv8.h) measurements on one MI355X; the shared pieces come from w4a16_probe.py.

  python profiles/kv8_probe.py attn [--reps 20]
      the target's verify attention at the 70B geometry (nh 64, nkv 8, hd 128, block 256, 8 query rows per sequence), ctx in {512, 2048,
      8192} x B in {1, 4}, launched exactly as HipDecoder.forward launches it (its own _attn_cfg / _attn_flags choice): ssd_attn_paged
      over a bf16 cache and ssd_attn_paged_fp8 over a byte cache alternating twice in the same process (bf16, fp8, bf16, fp8: the gap
      between the two bf16 passes is the spread a ratio is read against).  Every launch of a pass reads a different cache copy ("layer")
      and the copies of a pass add up to more than the 256 MiB Infinity Cache, as the 80 layers of a forward do.  HIP-event time per
      launch (with the split merge where the decomposition has one) and the K/V bytes it reads.
  python profiles/kv8_probe.py step [--kv fp8] [--steps 20 --warmup 5]
      the c4 workload exactly as w4a16_probe.py builds it with a bf16 target, with or without kv_cache_dtype="fp8": TTFT p50 at 128 and
      2048 prompt tokens, ms per step and the accepted length.
  python profiles/kv8_probe.py bytes
      (no GPU) KV bytes per token of the 70B target and the tokens that fit beside its bf16 weights in 288 GB at the default utilisation.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import w4a16_probe as P  # noqa: E402

PASSES = ("bf16", "fp8", "bf16", "fp8")
CACHE_FLOOR = 512 << 20          # bytes of K/V the launches of one pass read between two visits of the same copy
MAX_COPIES = 64


def attn(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import kv8_ops as KV8
    from ssd_amd.model import AttnMeta, HipDecoder
    from ssd_amd.model_config import PRESETS
    dev = torch.device("cuda", 0)
    cfg = dataclasses.replace(PRESETS["llama-3.1-70b"], num_layers=1, vocab_size=4096)
    nh, nkv, hd, bs, rows = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, 256, 8
    for ctx in (512, 2048, 8192):
        for B in (1, 4):
            T = B * rows
            mb = ctx // bs
            dec = HipDecoder(cfg, max_tokens=64, max_seqs=B, max_blocks=mb, block_size=bs, max_model_len=ctx, device=dev)
            bt = torch.arange(B * mb, dtype=torch.int32, device=dev).view(B, mb)
            meta = AttnMeta(H.MODE_CAUSAL, B, rows, torch.zeros(T, dtype=torch.int32, device=dev),
                            torch.full((B,), ctx, dtype=torch.int32, device=dev), bt, q_per_seq=rows, ctx_hint=ctx)
            splits, waves = dec._attn_cfg(T, meta)
            flags = dec._attn_flags(meta)
            q = torch.randn(T, nh * hd, device=dev).to(torch.bfloat16)
            scale = hd ** -0.5
            ks = torch.ones(nkv, dtype=torch.float32, device=dev)
            res = {}
            for i, dtype in enumerate(PASSES):
                elt = 1 if dtype == "fp8" else 2
                kv_bytes = 2 * B * ctx * nkv * hd * elt
                copies = max(2, min(MAX_COPIES, -(-CACHE_FLOOR // kv_bytes)))
                shape = (copies, 2, B * mb, nkv, bs, hd)
                if dtype == "fp8":      # finite codes: |value| <= 1.875 (exponent field <= 7)
                    kv = torch.randint(0, 0x40, shape, dtype=torch.uint8, device=dev) | (torch.randint(0, 2, shape, dtype=torch.uint8, device=dev) << 7)
                else:
                    kv = torch.randn(shape, device=dev).to(torch.bfloat16)

                def run():
                    for c in range(copies):
                        if dtype == "fp8":
                            KV8.attn_paged_fp8(q, kv[c, 0], kv[c, 1], bt, mb, meta.context_lens, B, T, rows, nh, nkv, hd, bs, scale, k_scale=ks,
                                               v_scale=ks, q_per_seq=rows, splits=splits, flags=flags, ws_o=dec.ws_o, ws_ml=dec.ws_ml,
                                               out_frag=dec.buf_af, waves=waves)
                        else:
                            H.attn_paged(q, kv[c, 0], kv[c, 1], bt, mb, meta.context_lens, B, T, rows, nh, nkv, hd, bs, scale, q_per_seq=rows,
                                         splits=splits, flags=flags, ws_o=dec.ws_o, ws_ml=dec.ws_ml, out_frag=dec.buf_af, waves=waves)
                us = P._time(run, args.reps) / copies
                res.setdefault(dtype, []).append(us)
                print(json.dumps({"probe": "verify_attn", "ctx": ctx, "B": B, "rows": rows, "splits": splits, "waves": waves, "flags": flags,
                                  "dtype": dtype, "pass": i, "copies": copies, "us": round(us, 2), "kv_bytes": kv_bytes,
                                  "GBs": round(kv_bytes / (us * 1e-6) / 1e9, 1)}), flush=True)
                del kv
                torch.cuda.empty_cache()
            b, f = sum(res["bf16"]) / 2, sum(res["fp8"]) / 2
            print(json.dumps({"probe": "verify_attn_ratio", "ctx": ctx, "B": B, "bf16_us": round(b, 2), "fp8_us": round(f, 2),
                              "fp8_over_bf16": round(f / b, 4), "bf16_spread": round(abs(res["bf16"][0] - res["bf16"][1]) / b, 4),
                              "fp8_spread": round(abs(res["fp8"][0] - res["fp8"][1]) / f, 4)}), flush=True)
            del dec
            torch.cuda.empty_cache()


def step(args):
    args.quant = "none"
    print(json.dumps({"probe": "mode", "quant": "none", "kv_cache_dtype": args.kv}), flush=True)
    P.step(args, engine_kw={"kv_cache_dtype": "fp8"} if args.kv == "fp8" else None)


def kv_bytes(args):
    from ssd_amd.model_config import PRESETS
    cfg = PRESETS["llama-3.1-70b"]
    weights = 139006066688           # HipDecoder.weight_bytes() of the bf16 70B target (profiles/fp8_step_bf16.jsonl)
    hbm, util = 288e9, 0.7
    for dtype, elt in (("bf16", 2), ("fp8", 1)):
        per_tok = 2 * cfg.num_layers * cfg.num_kv_heads * cfg.head_dim * elt
        print(json.dumps({"probe": "kv_bytes", "model": "llama-3.1-70b", "kv_cache_dtype": dtype, "bytes_per_token": per_tok,
                          "KiB_per_token": per_tok / 1024, "verify_read_GB_ctx8192_b1": round(per_tok * 8192 / 1e9, 3),
                          "verify_read_GB_ctx8192_b4": round(4 * per_tok * 8192 / 1e9, 3),
                          "tokens_beside_bf16_weights_at_0.7_of_free": int((hbm - weights) * util // per_tok)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["attn", "step", "bytes"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ttft-samples", type=int, default=5)
    a = ap.parse_args()
    with torch.inference_mode():
        {"attn": attn, "step": step, "bytes": kv_bytes}[a.mode](a)
