"""Sliding-window attention (include/ssd_hip_swa.h) measurements on one MI355X.

  python profiles/swa_probe.py [--passes 5 --launches 200]
      ssd_attn_paged_window against ssd_attn_paged on the same bf16 cache at Mistral-7B's geometry (nh 32, nkv 8, hd 128, block 256,
      one sequence): decode (1 row) and verify (8 rows) at ctx 4096, 8192 and 32768 under W = 4096, each launched with the decomposition
      HipDecoder._attn_cfg gives it (the windowed launch sizes its key splits from min(ctx bucket, W + rows)).  Every launch of a graph
      reads another copy of the cache and the copies add up to more than the 256 MiB Infinity Cache.  hipGraph replays, the two versions
      alternating, the median of `passes` timings each; the spread is (max - min) / median of a version's own timings.  At ctx 4096 no
      key is cut off: that ratio is to be read against the unwindowed kernel's own spread.
Prints one JSON line per shape."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from moe_probe import _graph  # noqa: E402
from moe_mx4_probe import _time  # noqa: E402

W = 4096
COLD_BYTES = 512 << 20


def main(args):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import swa_ops as SWA
    from ssd_amd.model import AttnMeta, HipDecoder
    from ssd_amd.model_config import presets
    dev = torch.device("cuda", 0)
    cfg = dataclasses.replace(presets()["mistral-7b-v0.1"], num_layers=1, vocab_size=4096)
    nh, nkv, hd, bs = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, 256
    scale = hd ** -0.5
    for ctx in (4096, 8192, 32768):
        mb = ctx // bs
        dec = HipDecoder(cfg, max_tokens=64, max_seqs=1, max_blocks=mb, block_size=bs, max_model_len=ctx, device=dev)
        kv_bytes = 2 * ctx * nkv * hd * 2
        copies = max(2, -(-COLD_BYTES // kv_bytes))
        kv = torch.randn(copies, 2, mb, nkv, bs, hd, device=dev).to(torch.bfloat16)
        bt = torch.arange(mb, dtype=torch.int32, device=dev).view(1, mb)
        for rows in (1, 8):
            meta = AttnMeta(H.MODE_CAUSAL, 1, rows, torch.zeros(rows, dtype=torch.int32, device=dev),
                            torch.full((1,), ctx, dtype=torch.int32, device=dev), bt, q_per_seq=rows, ctx_hint=ctx)
            (s_full, waves), s_win = dec._attn_cfg(rows, meta), dec._attn_cfg(rows, meta, W)[0]
            q = torch.randn(rows, nh * hd, device=dev).to(torch.bfloat16)
            kw = dict(q_per_seq=rows, ws_o=dec.ws_o, ws_ml=dec.ws_ml, out_frag=dec.buf_af, waves=waves)

            def full():
                for c in range(copies):
                    H.attn_paged(q, kv[c, 0], kv[c, 1], bt, mb, meta.context_lens, 1, rows, rows, nh, nkv, hd, bs, scale, splits=s_full, **kw)

            def window():
                for c in range(copies):
                    SWA.attn_paged_window(q, kv[c, 0], kv[c, 1], bt, mb, meta.context_lens, 1, rows, rows, nh, nkv, hd, bs, scale,
                                          splits=s_win, window=W, **kw)
            graphs = {"full": _graph(full), "window": _graph(window)}
            torch.cuda.synchronize()
            times = {v: [] for v in graphs}
            for _ in range(args.passes):
                for v, gr in graphs.items():
                    times[v].append(_time(gr, args.launches, copies))
            us = {v: statistics.median(t) for v, t in times.items()}
            seen = min(ctx, W + rows - 1)           # keys some row of the launch sees
            print(json.dumps({"probe": "swa_attn", "ctx": ctx, "rows": rows, "window": W, "waves": waves, "splits_full": s_full,
                              "splits_window": s_win, "copies": copies, "full_us": round(us["full"], 2), "window_us": round(us["window"], 2),
                              "full_spread": round((max(times["full"]) - min(times["full"])) / us["full"], 4),
                              "window_spread": round((max(times["window"]) - min(times["window"])) / us["window"], 4),
                              "time_ratio": round(us["window"] / us["full"], 4), "bytes_ratio": round(seen / ctx, 4)}), flush=True)
            del graphs
        del kv, dec
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    with torch.inference_mode():
        main(ap.parse_args())
