"""The tiled expert GEMM over MXFP4 tables against the weight-streaming one on one MI355X (csrc/moe_tiled.hip, MX4 form, vs
csrc/moe_mxfp4.hip): profiles/moe_tiled_probe.py's protocol over "mx4 frag" tables.

  python profiles/moe_tiled_mx4_probe.py [--pass-ms 40 --passes 5]
      the qwen3-30b-a3b expert shapes (h 2048, width 768) and the qwen3-235b-a22b ones (h 4096, width 1536), 128 experts, top 8,
      uniform random routes, T = 128, 256, 512, 1024, 2048, 8192: ssd_moe_gemm_mxfp4 and ssd_moe_gemm_tiled_mxfp4 on the SAME routes,
      rows and tables (random codes, scale bytes 116 .. 121), the up and the down GEMM each captured as a hipGraph of its own and
      replayed, the versions alternating pass by pass in one process, medians of the passes.  A graph walks enough copies of the
      tables that one replay touches at least COLD_BYTES (1 GiB of codes + scale bytes, four times the 256 MiB Infinity Cache), so no
      kernel is fed from the cache between replays.  A pass is as many replays as fill --pass-ms.  TF/s = 2 T k N K / time.
Prints one JSON line per (shapes, T, GEMM); "wins" applies HipDecoder.MOE_TILED_MX4_MIN_T's rule to the line: the tiled kernel's margin
exceeds the streaming kernel's own doubled spread."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from moe_probe import _graph, E_, K_  # noqa: E402
from moe_tiled_probe import COLD_BYTES, SHAPES, _time  # noqa: E402


def main(args):
    from ssd_amd.hip import moe_ops as M
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    for model, (h, I) in SHAPES.items():
        if args.model and model != args.model:
            continue
        # mx4 frag tables: any codes do, and any scale bytes that keep the sums finite
        tabs = {name: (torch.randint(0, 256, (E_ * N * K // 2,), generator=g, device=dev, dtype=torch.uint8),
                       torch.randint(116, 122, (E_ * N * K // 32,), generator=g, device=dev, dtype=torch.uint8))
                for name, N, K in (("up", 2 * I, h), ("down", h, I))}
        for T in (128, 256, 512, 1024, 2048, 8192):
            ids = torch.rand(T, E_, generator=g, device=dev).topk(K_, dim=-1).indices
            flat = ids.reshape(-1)
            perm = torch.sort(flat, stable=True).indices.int()
            offs = torch.zeros(E_ + 1, dtype=torch.int32, device=dev)
            offs[1:] = torch.bincount(flat, minlength=E_).cumsum(0).int()
            touched = int(torch.unique(flat).numel())
            x = torch.randn(T, h, generator=g, device=dev).to(bf)
            act = [torch.zeros(T * K_, I, dtype=bf, device=dev) for _ in range(2)]
            d = [torch.zeros(T * K_, h, dtype=bf, device=dev) for _ in range(2)]
            for name, rows, outs, N, K, epi in (("up", x, act, 2 * I, h, M.EPI_UP), ("down", act[0], d, h, I, M.EPI_DOWN)):
                copies = max(2, -(-COLD_BYTES // (touched * N * K * 17 // 32)))
                qs = [tabs[name]] + [(tabs[name][0].clone(), tabs[name][1].clone()) for _ in range(copies - 1)]

                def version(fn, out):
                    def run():
                        for q, s in qs:
                            fn(rows, q, s, offs, perm, out, T, K_, E_, N, K, epi)
                    return _graph(run)
                graphs = {"stream": version(M.moe_gemm_mxfp4, outs[0]), "tiled": version(M.moe_gemm_tiled_mxfp4, outs[1])}
                torch.cuda.synchronize()
                diff = float((outs[0].float() - outs[1].float()).abs().max())
                times = {v: [] for v in graphs}
                reps = {v: max(1, int(args.pass_ms * 1e3 / (_time(fn, 1, copies) * copies))) for v, fn in graphs.items()}
                for _ in range(args.passes):
                    for v, fn in graphs.items():
                        times[v].append(_time(fn, reps[v], copies))
                rec = {"probe": "moe_tiled_mx4_gemm", "model": model, "gemm": name, "T": T, "experts_touched": touched, "copies": copies,
                       "max_abs_diff_to_stream": diff}
                flop = 2.0 * T * K_ * N * K
                for v, ts in times.items():
                    us = statistics.median(ts)
                    rec.update({f"{v}_us": round(us, 2), f"{v}_spread": round((max(ts) - min(ts)) / us, 4), f"{v}_TFps": round(flop / us / 1e6, 1)})
                rec["margin"] = round(1.0 - rec["tiled_us"] / rec["stream_us"], 4)
                rec["wins"] = rec["margin"] > 2 * rec["stream_spread"]
                print(json.dumps(rec), flush=True)
                del qs, graphs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass-ms", type=float, default=40.0)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--model", default="")
    with torch.inference_mode():
        main(ap.parse_args())
