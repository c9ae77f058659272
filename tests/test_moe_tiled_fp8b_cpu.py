"""include/ssd_hip_moe_tiled_fp8b.h, its ctypes table and the library's export agree (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_signature_and_symbol():
    from ssd_amd.hip.lib import build_library, lib_path
    from ssd_amd.hip.moe_ops import MOE_FP8B_SIGNATURES, MOE_TILED_FP8B_SIGNATURES, load_moe_tiled_fp8b_library
    if not os.path.exists(lib_path()):
        build_library()
    text = open(os.path.join(ROOT, "include", "ssd_hip_moe_tiled_fp8b.h")).read()
    names = sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", text, flags=re.M)))
    assert names == sorted(MOE_TILED_FP8B_SIGNATURES) == ["ssd_moe_gemm_tiled_fp8b"]
    assert MOE_TILED_FP8B_SIGNATURES["ssd_moe_gemm_tiled_fp8b"] == MOE_FP8B_SIGNATURES["ssd_moe_gemm_fp8b"] and len(MOE_FP8B_SIGNATURES["ssd_moe_gemm_fp8b"]) == 13
    assert hasattr(load_moe_tiled_fp8b_library(), "ssd_moe_gemm_tiled_fp8b")
    assert "ACCUMULATION ORDER (normative)" in text
