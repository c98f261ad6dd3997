"""GroupHost::fold_planes under AddressSanitizer and UndefinedBehaviorSanitizer, on the host: tests/c/fold_planes_san.cpp is a
stand-alone program (its own main, no device, no library) built from gmsm_group_host.h as plain C++ - host code only, the
device side of the compiler is told to stay unsanitized - under the address and undefined-behaviour sanitizers; it
folds fixed planes and compares with the sum built plane by plane. A sanitizer report or a mismatch is a non-zero exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_fold_planes_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "fold_planes_san")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "gnark-crypto_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "fold_planes_san.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.count(": ok") == 5 and "all ok" in r.stdout
