"""iop.Evaluate on one GPU: python tools/iop_expr.py [out.json] (default profiles/iop_expr.json).
One GPU session; run it under a time limit (timeout 300 python tools/iop_expr.py).

BN254, N = 2^22 elements per polynomial (the big domain of a 2^20 circuit), every polynomial its own device allocation. Each
row is the host clock around the blocking call of gmsm_iop_evaluate_expression (it ends in a stream synchronise), median of
`reps` after a warm-up call (kernel_ms: the kernel alone, stage slot 0 with gmsm_set_profiling(1), a run of its own), for two
expressions:
  quotient   the reference's TestQuotient numerator x1^2 x2 + x3 - x1^3: 3 inputs, 4 products
  gate       a PLONK-gate-shaped numerator ql l + qr r + qm l r + qo o + qk plus one POINT term (l w^i): 8 inputs, 6 products
             and the POINT's own
Beside each time two floors, both from numbers that do not come from the code under test:
  floor_copy_ms      the bytes the call must move, (inputs + 1) N 32, at the rate of a device-to-device copy of one polynomial
                     measured in the same run (torch's copy kernel; read plus write counted); the project holds no other
                     measured copy rate, bench.py's 8 TB/s is the public peak
  floor_products_ms  the program's products (MUL instructions, and one for each POINT) times N at the measured product rate
                     of profiles/peaks_r06.json (bn254_fp_mul: BN254's coordinate field has the limb count of its scalar field)
No threshold is set. There is no Go toolchain here, so no reference time stands next to these. No ratio is claimed."""
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gm = importlib.import_module("gnark-crypto_amd")

CURVE, LOGN = "bn254", 22


def quotient(i, x1, x2, x3):
    return x1 * x1 * x2 + x3 - x1 * x1 * x1


def gate(i, ql, qr, qm, qo, qk, l, r, o):
    return ql * l + qr * r + qm * l * r + qo * o + qk + l * i.point()


def canonical(rng, c, n):
    a = rng.integers(0, 2**64, size=(n, c.fr_limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (c.fr_bits - 64 * (c.fr_limbs - 1) - 1)) - 1)
    return a


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_ms(fn, reps):
    """the kernel alone: stage slot 0 of gmsm_get_stage_times with profiling on (HIP events on the call's stream), per call"""
    lib = gm._lib.load()
    lib.gmsm_set_profiling(1)
    try:
        for _ in range(reps):
            fn()
        ms, calls = (ctypes.c_double * 8)(), ctypes.c_ulong(0)
        lib.gmsm_get_stage_times(ms, 8, ctypes.byref(calls))
    finally:
        lib.gmsm_set_profiling(0)
    return ms[0] / max(1, calls.value)


def product_rate():
    try:
        return float(json.load(open(os.path.join(ROOT, "profiles", "peaks_r06.json")))["bn254_fp_mul"])
    except (OSError, KeyError, ValueError):
        return None


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "iop_expr.json")
    reps = int(os.environ.get("IOP_EXPR_REPS", "9"))
    c = gm.CURVES[CURVE]
    n = 1 << LOGN
    rng = np.random.default_rng([0x10E, LOGN])
    stream = torch.cuda.current_stream().cuda_stream
    iop = gm.iop
    d = gm.fft.NewDomain(CURVE, n)
    try:
        polys = [torch.from_numpy(canonical(rng, c, n).view(np.int64).reshape(-1)).cuda() for _ in range(8)]
        d_out = torch.empty(n * c.fr_limbs, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def copy():
            d_out.copy_(polys[0])
            torch.cuda.synchronize()
        copy_ms = timed(copy, reps)
        bytes_poly = n * c.fr_limbs * 8
        copy_rate = 2 * bytes_poly / (copy_ms * 1e-3)  # bytes per second, read plus write
        rate = product_rate()
        out = {"tool": "tools/iop_expr.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE, "logn": LOGN,
               "copy": {"what": "torch device-to-device copy of one polynomial, host clock around copy + synchronise", "call_ms": copy_ms,
                        "bytes_per_s": copy_rate},
               "product_rate_per_s": rate, "product_rate_source": "profiles/peaks_r06.json bn254_fp_mul", "rows": []}
        for name, f, m in (("quotient", quotient, 3), ("gate", gate, 8)):
            code = iop.trace(CURVE, f, m)
            ops = [int(w) & 0xFF for w in code.words]
            products = ops.count(iop.EXPR_MUL) + ops.count(iop.EXPR_POINT)
            ptrs = [t.data_ptr() for t in polys[:m]]
            call = lambda: iop.evaluate_expression_device(CURVE, code, ptrs, n, [n] * m, [0] * m, [iop.Regular] * m, iop.Regular,
                                                          d_out.data_ptr(), domain=d if code.has_point else None, stream=stream)
            row = {"what": name, "inputs": m, "instructions": len(ops), "registers": len({(int(w) >> 8) & 0xFF for w in code.words}),
                   "products_per_index": products, "call_ms": timed(call, reps), "floor_copy_ms": (m + 1) * bytes_poly / copy_rate * 1e3}
            if rate:
                row["floor_products_ms"] = products * n / rate * 1e3
            row["kernel_ms"] = kernel_ms(call, reps)
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    finally:
        d.release()
        gm.trim(0)


if __name__ == "__main__":
    main()
