"""csrc/gemm.h: the L-axis descriptor builders of CubeMLP (gemm_lmul, gemm_lmul_t, gemm_lmul_dw and the two second-product forms) against
descriptors spelled out field by field, as a stand-alone host program under AddressSanitizer + UBSan.  CPU-only: no GPU call."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_laxis_builders_fill_exactly_their_fields(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    exe = str(tmp_path / "gemm_lmul")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    cmd = [hipcc, "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "--offload-arch=gfx950"] + \
          [a for f in san for a in ("-Xarch_host", f)] + \
          ["-I", os.path.join(ROOT, "mimrl_amd", "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "gemm_lmul_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "gemm builders ok" in r.stdout and "FAILED" not in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
