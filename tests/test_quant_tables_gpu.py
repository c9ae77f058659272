"""The device tables of every weight format, bit for bit: a tiny Llama target on synthetic weights (fixed seed) is loaded once per
variant -- each quantized decoder from bf16 linears and from its pre-quantized host types, and a bf16 decoder handed each of the five
host types -- and the SHA-256 of every tensor in dec.w (dtype, shape and bytes) is compared with tests/golden/quant_tables_sha.json.

A change to the loaders that is meant to leave behaviour alone must reproduce the digests.  The file holds names and digests only
and is written by this file's own record mode, on the GPU, from the tree whose tables are to be pinned:

    python tests/test_quant_tables_gpu.py --record          (QUANT_TABLES_OUT=<path> writes elsewhere)
"""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "quant_tables_sha.json")

# variant -> (HipDecoder keywords, the quantizer its decoder linears go through on the host; None: they arrive as bf16)
VARIANTS = {
    "fp8": (dict(quantization="fp8"), None),
    "fp8-from-block": (dict(quantization="fp8"), "quantize_fp8_block"),
    "w4a16": (dict(quantization="w4a16"), None),
    "w4a16-zero-point": (dict(quantization="w4a16", w4_zero_point=True), None),
    "w4a16-from-w4z": (dict(quantization="w4a16"), "quantize_w4a16_zp"),
    "mxfp4": (dict(quantization="mxfp4"), None),
    "bf16-from-fp8": ({}, "quantize_fp8"),
    "bf16-from-fp8-block": ({}, "quantize_fp8_block"),
    "bf16-from-w4": ({}, "quantize_w4a16"),
    "bf16-from-w4z": ({}, "quantize_w4a16_zp"),
    "bf16-from-mx4": ({}, "quantize_mxfp4"),
}


@functools.lru_cache(maxsize=None)
def _state():
    from ssd_amd import weights as W
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    return cfg, W.synthetic_state_dict(cfg, seed=3, std=0.05)


def table_digests(variant: str, device) -> dict:
    """name -> SHA-256 of every tensor the variant's decoder holds after load_weights."""
    from ssd_amd import quant
    from ssd_amd.model import HipDecoder
    kw, host = VARIANTS[variant]
    cfg, sd = _state()
    dec = HipDecoder(cfg, max_tokens=64, max_seqs=1, max_blocks=16, block_size=16, max_model_len=256, device=device, **kw)
    dec.load_weights((n, getattr(quant, host)(w) if host and quant.is_quantized_linear(n) else w) for n, w in sd.items())
    out = {}
    for name, t in sorted(dec.w.items()):
        t = t.detach().cpu().contiguous()
        head = f"{t.dtype}{list(t.shape)}".encode()
        out[name] = hashlib.sha256(head + t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_device_tables_are_the_recorded_ones(variant):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(FIXTURE) as f:
        want = json.load(f)
    assert set(want) == set(VARIANTS)
    got = table_digests(variant, torch.device("cuda", 0))
    assert set(got) == set(want[variant]), sorted(set(got) ^ set(want[variant]))
    assert len(got) >= 4 * 2 + 6
    differ = [n for n in got if got[n] != want[variant][n]]
    assert not differ, f"{variant}: {len(differ)} of {len(got)} tensors differ from the recording: {differ[:8]}"


if __name__ == "__main__":
    assert "--record" in sys.argv, "usage: python tests/test_quant_tables_gpu.py --record"
    out = os.environ.get("QUANT_TABLES_OUT", FIXTURE)
    rec = {v: table_digests(v, torch.device("cuda", 0)) for v in VARIANTS}
    assert rec == {v: table_digests(v, torch.device("cuda", 0)) for v in VARIANTS}, "two recordings differ"
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(rec)} variants, {sum(map(len, rec.values()))} tensors, {os.path.getsize(out)} bytes")
