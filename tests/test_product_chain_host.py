"""The Montgomery product scans of gmsm_fieldu.h (fpu_mul, fpu_mul_add, fpu_mul_add4, fpu_sqr and the two-at-once forms, on
unsigned and on signed limbs) compiled for the HOST and compared with big-integer arithmetic: tests/c/product_chain_check.cpp,
a stand-alone program (its own main, no device, no library) built once under the address and undefined-behaviour
sanitizers - a signed 64-bit column that overflows is undefined behaviour, which is what the second one reports. Operands:
every limb at the admitted extreme with the top limb at the call sites' bound, 0, 1, q - 1, q, 2q - 1, and 10 000 random
pairs per field. No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_product_scans_match_big_integers_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("ROCm clang++ not found")
    exe = str(tmp_path / "product_chain_check")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                    "-D__host__=", "-D__device__=", "-D__noinline__=", "-D__forceinline__=inline",
                    "-o", exe, os.path.join(ROOT, "tests", "c", "product_chain_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.count(" 0 mismatches") == 6, r.stdout
