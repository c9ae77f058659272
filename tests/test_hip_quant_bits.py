"""The weight-quantized GEMMs (csrc/gemm_wq.h and its four formats) give the bits they gave before they shared one kernel skeleton.

Every case of the case tables of tests/test_hip_quant_edges.py (`table(fmt)` for fp8, w4a16 and mxfp4) and of
tests/test_hip_w4zp_edges.py (the same table through the zero-point adapter) is run once: the inputs come from a seeded CPU
generator and are copied to the device, the call the table names (the default dispatch, or the _cfg form with the case's nt / deep /
waves / tpw) writes into a sentinel-filled buffer, and the SHA-256 of the whole buffer -- sentinels included, so a stray store shows
too -- is compared with tests/golden/quant_gemm_bits.json.  The fixture also holds the SHA-256 of every input (weights per (N, K),
x per (M, K), bias per (N, epilogue)) and of the table itself, so a changed generator or table fails saying so, before any kernel
is blamed.

The fixture was recorded on the MI355X from a build of the commit before the shared skeleton (`python tests/test_hip_quant_bits.py
OUT.json` in that tree: the recorder uses only the case tables, their adapters and the public *_ops calls), twice, with equal
results.  Many cases give equal bits (runs that differ only in tiles per workgroup, idle waves at a small K), so the fixture
stores, per format, the distinct 32-byte digests once (base64, in order of first appearance) and one index per case in table
order (uint16, zlib, base64); the input hashes are shared by the formats that share an input."""
from __future__ import annotations

import base64
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ssd_amd.hip.ops import EPI_ROWS, EPI_SILU_FRAG  # noqa: E402
from tests import test_hip_quant_edges as E  # noqa: E402
from tests.test_hip_mxfp4 import dev  # noqa: E402,F401  (the fixture)
from tests.test_hip_w4zp_edges import ZP  # noqa: E402

gpu = pytest.mark.gpu
BF = torch.bfloat16
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_gemm_bits.json")
ALL = {**E.FORMATS, ZP.name: ZP}
FMT = pytest.mark.parametrize("fmt", list(ALL.values()), ids=list(ALL))
SILU_TAIL = 4096                          # sentinel elements past the SILU fragment


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:7], "little"))


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _weights(fmt, N, K):
    """CPU tensors in the `rows` form the format's adapter takes (None where its frag() does not look), and those that matter."""
    g = _gen("w", fmt.name, N, K)
    if fmt.name == "fp8":                 # every e4m3fn code but the two NaNs (0x7f, 0xff); fp32 row scales of a 0.02-std weight's size
        c = torch.randint(0, 254, (N, K), generator=g, dtype=torch.uint8)
        c += (c >= 127).to(torch.uint8)
        s = torch.rand(N, generator=g) * 1e-3 + 1e-4
        return (c, s), (c, s)
    if fmt.name == "mxfp4":               # all 256 code pairs, scale bytes 117..123
        p = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
        s = torch.randint(117, 124, (N, K // 32), generator=g, dtype=torch.uint8)
        return (p, s), (p, s)
    p = torch.randint(-2 ** 31, 2 ** 31, (N, K // 8), generator=g, dtype=torch.int32)      # eight 4-bit codes per word, all values
    s = (torch.rand(N, K // 128, generator=g) * 6e-3 + 2e-3).to(BF)
    if fmt.name == "w4a16":
        return (None, s, p), (p, s)
    z = torch.randint(0, 16, (N, K // 128), generator=g, dtype=torch.uint8)
    return (None, s, z, p), (p, s, z)


class _Run:
    """Inputs of one format, built once per key on the CPU, hashed, and kept on the device while their (N, K) lasts."""

    def __init__(self, fmt, dev):
        self.fmt, self.dev, self.shape, self.hashes = fmt, dev, None, {}
        self.xs, self.biases = {}, {}

    def _at(self, N, K):
        if self.shape == (N, K):
            return
        self.rows = self.frags = None
        torch.cuda.empty_cache()
        rows, hashed = _weights(self.fmt, N, K)
        self.hashes[f"w {self.fmt.name} {N} {K}"] = _sha(*hashed)
        self.rows = tuple(None if t is None else t.to(self.dev) for t in rows)
        self.shape, self.frags = (N, K), {}

    def frag(self, c):
        from ssd_amd.quant import gate_up_row_map
        silu = c.epilogue == EPI_SILU_FRAG
        if silu not in self.frags:
            rmap = gate_up_row_map(c.N).to(self.dev) if silu else None
            self.frags[silu] = self.fmt.frag(self.rows, c.N, c.K, self.dev, rmap)
        return self.frags[silu]

    def x(self, c):
        from ssd_amd.hip import ops as H
        if (c.M, c.K) not in self.xs:
            x = torch.randn(c.M, c.K, generator=_gen("x", c.M, c.K)).to(BF)
            self.hashes[f"x {c.M} {c.K}"] = _sha(x)
            xf = torch.zeros(H.frag_numel(c.M, c.K), dtype=BF, device=self.dev)     # padding rows are zero
            H.rows_to_frag(x.to(self.dev), xf, c.M, c.K)
            self.xs[(c.M, c.K)] = xf
        return self.xs[(c.M, c.K)]

    def bias(self, c):
        if not c.bias:
            return None
        if (c.N, c.epilogue) not in self.biases:
            b = (torch.randn(c.N, generator=_gen("b", c.N, c.epilogue)) * 0.1).to(BF)
            self.hashes[f"b {c.N} {c.epilogue}"] = _sha(b)
            self.biases[(c.N, c.epilogue)] = b.to(self.dev)
        return self.biases[(c.N, c.epilogue)]

    def digest(self, c) -> bytes:
        from ssd_amd.hip import ops as H
        self._at(c.N, c.K)
        if c.epilogue == EPI_ROWS:
            numel, ldy = (c.M + 15) // 16 * 16 * c.N, c.N
        else:
            numel, ldy = H.frag_numel(c.M, c.N // 2) + SILU_TAIL, 0
        yb = torch.full((numel,), E.SENTINEL, dtype=torch.int16, device=self.dev)
        cfg = None if not c.nt else (c.nt | (256 if c.deep else 0), c.waves | (c.tpw << 8))
        self.fmt.gemm(self.x(c), self.frag(c), yb.view(BF), c.M, c.N, c.K, ldy, c.epilogue, self.bias(c), cfg)
        return hashlib.sha256(yb.cpu().numpy().tobytes()).digest()


def _table_sha(cases) -> str:
    return hashlib.sha256(repr([tuple(c) for c in cases]).encode()).hexdigest()


def _wrap(b: bytes) -> list:
    t = base64.b64encode(b).decode()
    return [t[i:i + 160] for i in range(0, len(t), 160)]


def pack(digests: list) -> dict:
    """Per-case digests -> the distinct ones in order of first appearance, and one index per case."""
    first: dict = {}
    index = [first.setdefault(d, len(first)) for d in digests]
    assert len(first) < 65536
    return {"digests": _wrap(b"".join(first)), "index": _wrap(zlib.compress(b"".join(i.to_bytes(2, "little") for i in index), 9))}


def unpack(entry: dict) -> list:
    d, ix = base64.b64decode("".join(entry["digests"])), zlib.decompress(base64.b64decode("".join(entry["index"])))
    return [d[32 * i:32 * i + 32] for i in (int.from_bytes(ix[j:j + 2], "little") for j in range(0, len(ix), 2))]


def run_format(fmt, dev):
    """(per-case digests in table order, input hashes by key) of one format."""
    cases = E.table(fmt)
    order = sorted(range(len(cases)), key=lambda i: (cases[i].N, cases[i].K))      # one weight matrix on the device at a time
    run, digests = _Run(fmt, dev), [b""] * len(cases)
    for i in order:
        digests[i] = run.digest(cases[i])
    return digests, run.hashes


def _input_keys(fmt, cases) -> set:
    return ({f"w {fmt.name} {c.N} {c.K}" for c in cases} | {f"x {c.M} {c.K}" for c in cases}
            | {f"b {c.N} {c.epilogue}" for c in cases if c.bias})


def record(path: str) -> None:
    d = torch.device("cuda", 0)
    out = {"inputs": {}, "formats": {}}
    for name, fmt in ALL.items():
        digests, hashes = run_format(fmt, d)
        assert all(out["inputs"].setdefault(k, v) == v for k, v in hashes.items())
        out["formats"][name] = {"cases": len(digests), "table": _table_sha(E.table(fmt)), **pack(digests)}
    out["inputs"] = dict(sorted(out["inputs"].items()))
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(v['cases'] for v in out['formats'].values())} cases -> {path}")


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@FMT
def test_fixture_has_one_digest_for_every_case_of_the_table(fmt):
    fx, cases = _fixture(), E.table(fmt)
    want = fx["formats"][fmt.name]
    assert want["table"] == _table_sha(cases), f"{fmt.name}: the case table is not the one the fixture was recorded from"
    digests = unpack(want)
    assert want["cases"] == len(cases) == len(digests) and all(len(d) == 32 for d in digests)
    assert _input_keys(fmt, cases) <= set(fx["inputs"])
    assert set(fx["inputs"]) == set().union(*(_input_keys(f, E.table(f)) for f in ALL.values()))


@gpu
@FMT
def test_every_case_gives_the_recorded_bits(dev, fmt):
    fx, cases = _fixture(), E.table(fmt)
    want = fx["formats"][fmt.name]
    assert want["table"] == _table_sha(cases), f"{fmt.name}: the case table changed"
    got, hashes = run_format(fmt, dev)
    changed = [k for k, v in hashes.items() if fx["inputs"].get(k) != v]
    assert not changed and set(hashes) == _input_keys(fmt, cases), \
        f"{fmt.name}: inputs differ from the recording (the generator, not the kernel): {changed[:8]}"
    rec = unpack(want)
    bad = [i for i in range(len(cases)) if got[i] != rec[i]]
    print(f"{fmt.name}: {len(cases)} cases, {len(set(rec))} distinct outputs, {len(bad)} differ")
    assert not bad, f"{fmt.name}: kernel output bits differ from the recording in {len(bad)} of {len(cases)} cases, first {[cases[i] for i in bad[:4]]}"


if __name__ == "__main__":
    with torch.inference_mode():
        record(sys.argv[1])
