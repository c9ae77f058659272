"""(no GPU) The compiler's resource report of every weight-quantized GEMM instantiation, two trees side by side.

  python profiles/wq_resources.py PARENT_DIR NEW_DIR > profiles/wq_skeleton_resources.txt

Each directory holds gemm_fp8.txt, gemm_w4a16.txt and gemm_mxfp4.txt: the stderr of the Makefile's compile line for that file with
`--cuda-device-only -Rpass-analysis=kernel-resource-usage` added (profiles/wq_skeleton_commands.txt).  Kernels are matched by format
and template arguments (MT, NT, EPI, U, XS): gemm_fp8_kernel<MT, NT, EPI, U> is XS = true, gemm_w4a16_kernel's last argument is the
zero-point form.  Exits 1 if the sets differ, if scratch appears where the first tree has none, if occupancy differs, or if a kernel
of the second tree is above 256 VGPRs."""
from __future__ import annotations

import os
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def _key(name: str):
    m = re.match(r"void (\w+)<(.*)>\(", name)
    if not m or "gemm" not in m.group(1) or m.group(1).endswith(("frag_kernel", "rows_kernel")):
        return None
    kern, args = m.group(1), [a.strip() for a in re.sub(r"W4<(\w+)>", r"W4\1", m.group(2)).split(",")]
    as_bool = lambda a: a in ("true", "1")                      # noqa: E731
    if kern == "wq_gemm_kernel":
        fmt = {"Fp8": "fp8", "W4false": "w4a16", "W4true": "w4a16_zp", "Mx4": "mxfp4"}[args[0]]
        mt, nt, epi, u = map(int, args[1:5])
        return fmt, mt, nt, epi, u, as_bool(args[5])
    mt, nt, epi, u = map(int, args[:4])
    if kern == "gemm_fp8_kernel":
        return "fp8", mt, nt, epi, u, True
    if kern == "gemm_w4a16_kernel":
        return ("w4a16_zp" if as_bool(args[5]) else "w4a16"), mt, nt, epi, u, as_bool(args[4])
    if kern == "gemm_mxfp4_kernel":
        return "mxfp4", mt, nt, epi, u, as_bool(args[4])
    return None


def read(d: str) -> dict:
    out, cur = {}, None
    for f in ("gemm_fp8.txt", "gemm_w4a16.txt", "gemm_mxfp4.txt"):
        for line in open(os.path.join(d, f)):
            m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True, check=True).stdout.strip()
                cur = _key(name)
                if cur is not None:
                    assert cur not in out, cur
                    out[cur] = {}
            elif cur is not None and m.group(1) in FIELDS:
                out[cur][m.group(1)] = int(m.group(2))
    return out


def main(a: str, b: str) -> int:
    A, B = read(a), read(b)
    bad = []
    if set(A) != set(B):
        bad.append(f"instantiation sets differ: only first {sorted(set(A) - set(B))}, only second {sorted(set(B) - set(A))}")
    print(f"{len(A)} / {len(B)} GEMM instantiations (first / second tree); columns are first -> second")
    print(f"{'format':9} {'MT':>2} {'NT':>2} {'EPI':>3} {'U':>2} {'XS':>2} | {'VGPRs':>10} {'AGPRs':>7} {'SGPRs':>10} {'scratch':>8} {'occup':>6} {'LDS':>6}  moved")
    for k in sorted(set(A) & set(B)):
        x, y = A[k], B[k]
        cell = lambda f: f"{x[f]}->{y[f]}"                   # noqa: E731
        moved = [f.split()[0] for f in FIELDS if x[f] != y[f]]
        print(f"{k[0]:9} {k[1]:>2} {k[2]:>2} {k[3]:>3} {k[4]:>2} {int(k[5]):>2} | {cell(FIELDS[0]):>10} {cell(FIELDS[1]):>7} {cell(FIELDS[2]):>10} "
              f"{cell(FIELDS[3]):>8} {cell(FIELDS[4]):>6} {cell(FIELDS[5]):>6}  {' '.join(moved)}")
        if x[FIELDS[3]] == 0 and y[FIELDS[3]] != 0:
            bad.append(f"{k}: scratch {y[FIELDS[3]]} where the first tree has none")
        if x[FIELDS[4]] != y[FIELDS[4]]:
            bad.append(f"{k}: occupancy {x[FIELDS[4]]} -> {y[FIELDS[4]]}")
        if y[FIELDS[0]] + y[FIELDS[1]] > 256:
            bad.append(f"{k}: {y[FIELDS[0]]} + {y[FIELDS[1]]} registers, above the 256 of a 512-thread workgroup")
    print("conditions: " + ("all hold (same set, no new scratch, equal occupancy, <= 256 VGPRs)" if not bad else "VIOLATED"))
    for line in bad:
        print("  " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
