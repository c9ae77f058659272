"""The grouped MXFP4 expert GEMM against the bf16 one on one MI355X (csrc/moe_mxfp4.hip vs csrc/moe.hip).

  python profiles/moe_mx4_probe.py [--launches 1000 --passes 5]
      the qwen3-30b-a3b shapes (h 2048, 128 experts of width 768, top 8): ssd_moe_gemm_mxfp4 and ssd_moe_gemm on the SAME routes and
      the SAME weights (random MXFP4 codes; the bf16 tables are their exact image from ssd_mx4_dequant_frag), the up and the down GEMM
      each captured as a hipGraph of its own and replayed, the two versions alternating pass by pass in one process.  T = 1, 8, 24
      with distinct experts per row (8 T experts touched), T = 2048 with uniform random routes (128 rows per expert on average: two
      64-row passes or more, and the mxfp4 kernel converts every code once per pass).  The number of table copies a graph walks is sized
      by BYTES, per version and per row of the table below: enough copies that one replay touches at least COLD_BYTES (1 GiB, four
      times the 256 MiB Infinity Cache) of expert tables, so neither kernel is fed from the cache between replays -- at T = 1 that is
      81 / 161 copies of the mxfp4 up / down tables and 22 / 43 of the bf16 ones.  Bytes = the tables of the experts touched (codes +
      scale bytes, or bf16), activations not counted.
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

COLD_BYTES = 1 << 30


def _time(fn, launches, copies):
    """us per GEMM launch over whole replays of a graph of `copies` launches."""
    reps = max(1, launches // copies)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / (reps * copies)


def _tables(N, K, gate_up, g, dev):
    """(mx4 frag codes, frag scale bytes, bf16 frag image) of E_ random matrices [N][K]."""
    from ssd_amd import quant
    from ssd_amd.hip import mx4_ops as MX
    qb, sb = N * K // 2, N * K // 32
    q = torch.empty(E_ * qb, dtype=torch.uint8, device=dev)
    s = torch.empty(E_ * sb, dtype=torch.uint8, device=dev)
    w = torch.empty(E_ * N * K, dtype=torch.bfloat16, device=dev)
    row_map = quant.gate_up_row_map(N).to(dev) if gate_up else None
    for e in range(E_):
        packed = torch.randint(0, 256, (N, K // 2), generator=g, device=dev, dtype=torch.uint8)
        scale = torch.randint(116, 122, (N, K // 32), generator=g, device=dev, dtype=torch.uint8)
        MX.mx4_rows_to_frag(packed, scale, q[e * qb:(e + 1) * qb], s[e * sb:(e + 1) * sb], N, K, row_map=row_map)
        MX.mx4_dequant_frag(q[e * qb:(e + 1) * qb], s[e * sb:(e + 1) * sb], w[e * N * K:(e + 1) * N * K], N, K)
    return q, s, w


def main(args):
    from ssd_amd.hip import moe_ops as M
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    up, dn = _tables(2 * I_, H_, True, g, dev), _tables(H_, I_, False, g, dev)
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
        act = [torch.zeros(T * K_, I_, dtype=bf, device=dev) for _ in range(2)]
        d = [torch.zeros(T * K_, H_, dtype=bf, device=dev) for _ in range(2)]
        for name, (q0, s0, w0), rows, outs, N, K, epi in (("up", up, x, act, 2 * I_, H_, M.EPI_UP), ("down", dn, act[0], d, H_, I_, M.EPI_DOWN)):
            wb = touched * N * K
            cm, cb = max(2, -(-COLD_BYTES // (wb * 17 // 32))), max(2, -(-COLD_BYTES // (wb * 2)))
            qs = [(q0, s0)] + [(q0.clone(), s0.clone()) for _ in range(cm - 1)]
            ws = [w0] + [w0.clone() for _ in range(cb - 1)]

            def mx4():
                for q, s in qs:
                    M.moe_gemm_mxfp4(rows, q, s, offs, perm, outs[0], T, K_, E_, N, K, epi)

            def bf16():
                for w in ws:
                    M.moe_gemm(rows, w, offs, perm, outs[1], T, K_, E_, N, K, epi)
            gm, gb = _graph(mx4), _graph(bf16)
            torch.cuda.synchronize()
            tm, tb = [], []
            for _ in range(args.passes):
                tb.append(_time(gb, args.launches, cb))
                tm.append(_time(gm, args.launches, cm))
            m_us, b_us = statistics.median(tm), statistics.median(tb)
            del qs, ws, gm, gb
            torch.cuda.empty_cache()
            print(json.dumps({"probe": "moe_mx4_gemm", "gemm": name, "T": T, "experts_touched": touched, "copies_mxfp4": cm, "copies_bf16": cb,
                              "mxfp4_us": round(m_us, 2), "mxfp4_spread": round((max(tm) - min(tm)) / m_us, 4),
                              "bf16_us": round(b_us, 2), "bf16_spread": round((max(tb) - min(tb)) / b_us, 4),
                              "time_ratio": round(m_us / b_us, 4), "bytes_ratio": round(17 / 64, 4),
                              "mxfp4_TBps": round(wb * 17 / 32 / m_us / 1e6, 3), "bf16_TBps": round(wb * 2 / b_us / 1e6, 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=5)
    with torch.inference_mode():
        main(ap.parse_args())
