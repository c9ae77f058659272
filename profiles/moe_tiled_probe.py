"""The tiled expert GEMM against the weight-streaming one on one MI355X (csrc/moe_tiled.hip vs csrc/moe.hip).

  python profiles/moe_tiled_probe.py [--pass-ms 40 --passes 5]
      the qwen3-30b-a3b expert shapes (h 2048, width 768) and the qwen3-235b-a22b ones (h 4096, width 1536), 128 experts, top 8,
      uniform random routes, T = 128, 256, 512, 1024, 2048, 8192: ssd_moe_gemm and ssd_moe_gemm_tiled on the SAME
      routes, rows and tables, the up and the down GEMM each captured as a hipGraph of its own and replayed, the versions alternating
      pass by pass in one process, medians of the passes.  A graph walks enough copies of the tables that one replay touches at
      least COLD_BYTES (1 GiB, four times the 256 MiB Infinity Cache), so no kernel is fed from the cache between replays.  A pass
      is as many replays as fill --pass-ms.  TF/s = 2 T k N K / time.
Prints one JSON line per (shapes, T, GEMM)."""
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

COLD_BYTES = 1 << 30
SHAPES = {"qwen3-30b-a3b": (2048, 768), "qwen3-235b-a22b": (4096, 1536)}


def _time(fn, reps, copies):
    """us per GEMM launch over `reps` replays of a graph of `copies` launches."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / (reps * copies)


def main(args):
    from ssd_amd.hip import moe_ops as M
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    for model, (h, I) in SHAPES.items():
        if args.model and model != args.model:
            continue
        # frag-major tables: any bits do
        tabs = {"up": (torch.randn(E_ * 2 * I * h // 8, generator=g, device=dev) * 0.02).to(bf).repeat(8),
                "down": (torch.randn(E_ * h * I // 8, generator=g, device=dev) * 0.02).to(bf).repeat(8)}
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
                copies = max(2, -(-COLD_BYTES // (touched * N * K * 2)))
                ws = [tabs[name]] + [tabs[name].clone() for _ in range(copies - 1)]

                def version(fn, out):
                    def run():
                        for w in ws:
                            fn(rows, w, offs, perm, out, T, K_, E_, N, K, epi)
                    return _graph(run)
                graphs = {"stream": version(M.moe_gemm, outs[0]), "tiled": version(M.moe_gemm_tiled, outs[1])}
                torch.cuda.synchronize()
                diff = float((outs[0].float() - outs[1].float()).abs().max())
                times = {v: [] for v in graphs}
                reps = {v: max(1, int(args.pass_ms * 1e3 / (_time(fn, 1, copies) * copies))) for v, fn in graphs.items()}
                for _ in range(args.passes):
                    for v, fn in graphs.items():
                        times[v].append(_time(fn, reps[v], copies))
                rec = {"probe": "moe_tiled_gemm", "model": model, "gemm": name, "T": T, "experts_touched": touched, "copies": copies,
                       "max_abs_diff_to_stream": diff}
                flop = 2.0 * T * K_ * N * K
                for v, ts in times.items():
                    us = statistics.median(ts)
                    rec.update({f"{v}_us": round(us, 2), f"{v}_spread": round((max(ts) - min(ts)) / us, 4), f"{v}_TFps": round(flop / us / 1e6, 1)})
                print(json.dumps(rec), flush=True)
                del ws, graphs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass-ms", type=float, default=40.0)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--model", default="")
    with torch.inference_mode():
        main(ap.parse_args())
