"""The grouped block-scaled FP8 expert GEMM against the bf16 and the MXFP4 ones on one MI355X (csrc/moe_fp8b.hip vs csrc/moe.hip and
csrc/moe_mxfp4.hip).

  python profiles/moe_fp8b_probe.py [--launches 1000 --passes 5]
      the protocol of profiles/moe_mx4_probe.py at the qwen3-30b-a3b shapes (h 2048, 128 experts of width 768, top 8):
      ssd_moe_gemm_fp8b, ssd_moe_gemm and ssd_moe_gemm_mxfp4 on the SAME routes (the fp8 and bf16 kernels on the same weights: random
      e4m3 codes with scales 2^U(-9,-5) * U(1,2), the bf16 tables their image from ssd_fp8b_dequant_frag; the mxfp4 tables are random
      codes of their own), the up and the down GEMM each captured as a hipGraph of its own and replayed, the three versions alternating
      pass by pass in one process.  T = 1, 8, 24 with distinct experts per row, T = 2048 with uniform random routes.  The number of
      table copies a graph walks is sized by BYTES, per version: enough copies that one replay touches at least COLD_BYTES (1 GiB, four
      times the 256 MiB Infinity Cache) of expert tables.  Bytes = the tables of the experts touched (codes + scales, or bf16),
      activations not counted.
Prints one JSON line per (T, GEMM)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from moe_probe import _graph, H_, I_, E_, K_  # noqa: E402
from moe_mx4_probe import _time, _tables as _mx4_tables, COLD_BYTES  # noqa: E402

F8_BYTES = 1 + 4 / (16 * 128)       # per weight: one code byte + one fp32 scale per 16 rows x 128 columns


def _tables(N, K, gate_up, g, dev):
    """(fp8 frag codes, group scales fp32, bf16 frag image) of E_ random matrices [N][K]."""
    from ssd_amd import quant
    from ssd_amd.hip import fp8b_ops as F8B, quant_ops as Q
    q = torch.empty(E_ * N * K, dtype=torch.uint8, device=dev)
    s = torch.exp2(4.0 * torch.rand(E_ * (N // 16) * (K // 128), generator=g, device=dev) - 9.0) \
        * (1.0 + torch.rand(E_ * (N // 16) * (K // 128), generator=g, device=dev))
    w = torch.empty(E_ * N * K, dtype=torch.bfloat16, device=dev)
    row_map = quant.gate_up_row_map(N).to(dev) if gate_up else None
    sb = (N // 16) * (K // 128)
    for e in range(E_):
        codes = torch.randint(0, 127, (N, K), generator=g, device=dev, dtype=torch.uint8)
        codes |= torch.randint(0, 2, (N, K), generator=g, device=dev, dtype=torch.uint8) << 7
        Q.fp8_rows_to_frag(codes, q[e * N * K:(e + 1) * N * K], N, K, row_map=row_map)
        F8B.fp8b_dequant_frag(q[e * N * K:(e + 1) * N * K], s[e * sb:(e + 1) * sb], w[e * N * K:(e + 1) * N * K], N, K)
    return q, s, w


def main(args):
    from ssd_amd.hip import moe_ops as M
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    up, dn = _tables(2 * I_, H_, True, g, dev), _tables(H_, I_, False, g, dev)
    up4, dn4 = _mx4_tables(2 * I_, H_, True, g, dev)[:2], _mx4_tables(H_, I_, False, g, dev)[:2]
    for T in (1, 8, 24, 2048):
        if T * K_ <= E_:
            ids = torch.randperm(E_, generator=g, device=dev)[:T * K_].view(T, K_)
        elif T <= 24:       # 24 rows: 192 choices over 128 experts, distinct within a row
            ids = torch.stack([(torch.arange(K_, device=dev) + K_ * t) % E_ for t in range(T)])
        else:
            ids = torch.rand(T, E_, generator=g, device=dev).topk(K_, dim=-1).indices
        flat = ids.reshape(-1)
        perm = torch.sort(flat, stable=True).indices.int()
        offs = torch.zeros(E_ + 1, dtype=torch.int32, device=dev)
        offs[1:] = torch.bincount(flat, minlength=E_).cumsum(0).int()
        touched = int(torch.unique(flat).numel())
        x = torch.randn(T, H_, generator=g, device=dev).to(bf)
        act = [torch.zeros(T * K_, I_, dtype=bf, device=dev) for _ in range(3)]
        d = [torch.zeros(T * K_, H_, dtype=bf, device=dev) for _ in range(3)]
        for name, (q0, s0, w0), (p0, b0), rows, outs, N, K, epi in (("up", up, up4, x, act, 2 * I_, H_, M.EPI_UP),
                                                                    ("down", dn, dn4, act[0], d, H_, I_, M.EPI_DOWN)):
            wb = touched * N * K
            copies = {"fp8b": max(2, -(-COLD_BYTES // int(wb * F8_BYTES))), "bf16": max(2, -(-COLD_BYTES // (wb * 2))),
                      "mxfp4": max(2, -(-COLD_BYTES // (wb * 17 // 32)))}
            qs = [(q0, s0)] + [(q0.clone(), s0.clone()) for _ in range(copies["fp8b"] - 1)]
            ws = [w0] + [w0.clone() for _ in range(copies["bf16"] - 1)]
            ps = [(p0, b0)] + [(p0.clone(), b0.clone()) for _ in range(copies["mxfp4"] - 1)]

            def fp8b():
                for q, s in qs:
                    M.moe_gemm_fp8b(rows, q, s, offs, perm, outs[0], T, K_, E_, N, K, epi)

            def bf16():
                for w in ws:
                    M.moe_gemm(rows, w, offs, perm, outs[1], T, K_, E_, N, K, epi)

            def mxfp4():
                for q, s in ps:
                    M.moe_gemm_mxfp4(rows, q, s, offs, perm, outs[2], T, K_, E_, N, K, epi)
            graphs = {"bf16": _graph(bf16), "fp8b": _graph(fp8b), "mxfp4": _graph(mxfp4)}
            torch.cuda.synchronize()
            times = {v: [] for v in graphs}
            for _ in range(args.passes):
                for v, gr in graphs.items():
                    times[v].append(_time(gr, args.launches, copies[v]))
            us = {v: statistics.median(t) for v, t in times.items()}
            spread = {v: (max(t) - min(t)) / us[v] for v, t in times.items()}
            del qs, ws, ps, graphs
            torch.cuda.empty_cache()
            rec = {"probe": "moe_fp8b_gemm", "gemm": name, "T": T, "experts_touched": touched}
            for v in ("fp8b", "bf16", "mxfp4"):
                rec.update({f"copies_{v}": copies[v], f"{v}_us": round(us[v], 2), f"{v}_spread": round(spread[v], 4)})
            rec.update({"time_ratio": round(us["fp8b"] / us["bf16"], 4), "bytes_ratio": round(F8_BYTES / 2, 4),
                        "time_ratio_mxfp4": round(us["mxfp4"] / us["bf16"], 4),
                        "fp8b_TBps": round(wb * F8_BYTES / us["fp8b"] / 1e6, 3), "bf16_TBps": round(wb * 2 / us["bf16"] / 1e6, 3)})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=5)
    with torch.inference_mode():
        main(ap.parse_args())
