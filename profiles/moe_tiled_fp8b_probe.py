"""The tiled expert GEMM over block-scaled FP8 tables against the weight-streaming one on one MI355X (csrc/moe_tiled.hip, FP8B form,
vs csrc/moe_fp8b.hip): profiles/moe_tiled_mx4_probe.py's protocol over "fp8 frag" tables.

  python profiles/moe_tiled_fp8b_probe.py [--pass-ms 40 --passes 5]
      the qwen3-30b-a3b expert shapes (h 2048, width 768) and the qwen3-235b-a22b ones (h 4096, width 1536), 128 experts, top 8,
      uniform random routes, T = 128, 256, 512, 1024, 2048, 8192: ssd_moe_gemm_fp8b and ssd_moe_gemm_tiled_fp8b on the SAME routes,
      rows and tables (random finite codes, scales 2^-7 * U(1, 2)), the up and the down GEMM each captured as a hipGraph of its own
      and replayed, the versions alternating pass by pass in one process, medians of the passes.  A graph walks enough copies of the
      tables that one replay touches at least COLD_BYTES (1 GiB of codes + scales, four times the 256 MiB Infinity Cache), so no
      kernel is fed from the cache between replays.  A pass is as many replays as fill --pass-ms.  TF/s = 2 T k N K / time.
Prints one JSON line per (shapes, T, GEMM); "wins" applies HipDecoder.MOE_TILED_FP8B_MIN_T's rule to the line: the tiled kernel's
margin exceeds the streaming kernel's own doubled spread."""
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
        # fp8 frag tables: any finite codes do (0x7F / 0xFF are e4m3fn NaN), and scales that keep the sums finite
        tabs = {name: (torch.randint(0, 127, (E_ * N * K,), generator=g, device=dev, dtype=torch.uint8)
                       | (torch.randint(0, 2, (E_ * N * K,), generator=g, device=dev, dtype=torch.uint8) << 7),
                       (1.0 + torch.rand(E_ * (N // 16) * (K // 128), generator=g, device=dev)) / 128.0)
                for name, N, K in (("up", 2 * I, h), ("down", h, I))}
        for T in (128, 256, 512, 1024, 2048, 8192):
            if args.T and T not in args.T:
                continue
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
                copies = max(2, -(-COLD_BYTES // (touched * (N * K + N * K // 512))))
                qs = [tabs[name]] + [(tabs[name][0].clone(), tabs[name][1].clone()) for _ in range(copies - 1)]

                def version(fn, out):
                    def run():
                        for q, s in qs:
                            fn(rows, q, s, offs, perm, out, T, K_, E_, N, K, epi)
                    return _graph(run)
                graphs = {"stream": version(M.moe_gemm_fp8b, outs[0]), "tiled": version(M.moe_gemm_tiled_fp8b, outs[1])}
                torch.cuda.synchronize()
                diff = float((outs[0].float() - outs[1].float()).abs().max())
                times = {v: [] for v in graphs}
                reps = {v: max(1, int(args.pass_ms * 1e3 / (_time(fn, 1, copies) * copies))) for v, fn in graphs.items()}
                for _ in range(args.passes):
                    for v, fn in graphs.items():
                        times[v].append(_time(fn, reps[v], copies))
                rec = {"probe": "moe_tiled_fp8b_gemm", "model": model, "gemm": name, "T": T, "experts_touched": touched, "copies": copies,
                       "max_abs_diff_to_stream": diff, "max_abs_out": float(outs[0].float().abs().max())}
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
    ap.add_argument("--T", type=int, nargs="*", default=[])
    with torch.inference_mode():
        main(ap.parse_args())
