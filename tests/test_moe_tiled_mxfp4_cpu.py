"""include/ssd_hip_moe_tiled_mxfp4.h, its ctypes table and the library's export agree (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_signature_and_symbol():
    from ssd_amd.hip.lib import build_library, lib_path
    from ssd_amd.hip.moe_ops import MOE_MX4_SIGNATURES, MOE_TILED_MX4_SIGNATURES, load_moe_tiled_mx4_library
    if not os.path.exists(lib_path()):
        build_library()
    text = open(os.path.join(ROOT, "include", "ssd_hip_moe_tiled_mxfp4.h")).read()
    names = sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", text, flags=re.M)))
    assert names == sorted(MOE_TILED_MX4_SIGNATURES) == ["ssd_moe_gemm_tiled_mxfp4"]
    assert MOE_TILED_MX4_SIGNATURES["ssd_moe_gemm_tiled_mxfp4"] == MOE_MX4_SIGNATURES["ssd_moe_gemm_mxfp4"] and len(MOE_MX4_SIGNATURES["ssd_moe_gemm_mxfp4"]) == 13
    assert hasattr(load_moe_tiled_mx4_library(), "ssd_moe_gemm_tiled_mxfp4")
    assert "ACCUMULATION ORDER (normative)" in text and "bit-identical to ssd_moe_gemm_tiled" in text
