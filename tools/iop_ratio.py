"""The copy-constraint ratio polynomial on one GPU: python tools/iop_ratio.py [out.json] (default profiles/iop_ratio.json).
One GPU session; run it under a time limit (timeout 300 python tools/iop_ratio.py).

gmsm_iop_ratio_copy_constraint on BN254, n = 2^20, m = 3 wire polynomials in Lagrange / Regular form, a random permutation,
everything device-resident (entries, permutation and Z), with Z asked for as Lagrange / Regular (no transform) and as
Canonical / Regular (an inverse FFT and a bit reversal). Per form:
  call_ms     host clock around the blocking call (it ends in a stream synchronise), median of `reps` after a warm-up call
  stages_ms   the call's stages from gmsm_get_stage_times with profiling on (HIP events on the call's stream, a run of their
              own: the events cost a little): factors, scan (both prefix products), invert (inversion and final multiply),
              transforms (the expected form)
There is no Go toolchain here, so no reference time stands next to these; the nearest measured neighbour is the division
scan of the same length, copied from profiles/kzg_open.json (divide_ms of BN254 2^20, host-timed as well). No ratio is
claimed."""
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

CURVE, LOGN, M = "bn254", 20, 3
STAGE_SLOTS = {"factors": 0, "scan": 2, "invert": 5, "transforms": 6}  # include/gmsm.h, the ratio entries' profiling slots


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


def stage_times(fn, reps):
    lib = gm._lib.load()
    lib.gmsm_set_profiling(1)
    try:
        for _ in range(reps):
            fn()
        ms = (ctypes.c_double * 8)()
        calls = ctypes.c_ulong(0)
        lib.gmsm_get_stage_times(ms, 8, ctypes.byref(calls))
    finally:
        lib.gmsm_set_profiling(0)
    return {k: ms[i] / max(1, calls.value) for k, i in STAGE_SLOTS.items()}


def neighbour():
    try:
        rows = json.load(open(os.path.join(ROOT, "profiles", "kzg_open.json")))["rows"]
        row = next(r for r in rows if r["curve"] == CURVE and r["logn"] == LOGN)
        return {"source": "profiles/kzg_open.json", "what": "division by (X - a), the suffix scan of the same length", "divide_ms": row["divide_ms"]}
    except (OSError, KeyError, StopIteration):
        return None


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "iop_ratio.json")
    reps = int(os.environ.get("IOP_RATIO_REPS", "7"))
    c = gm.CURVES[CURVE]
    n = 1 << LOGN
    rng = np.random.default_rng([0x10B, LOGN])
    stream = torch.cuda.current_stream().cuda_stream
    iop = gm.iop
    out = {"tool": "tools/iop_ratio.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE, "logn": LOGN, "m": M,
           "nearest_measured_neighbour": neighbour(), "rows": []}
    d = gm.fft.NewDomain(CURVE, n)
    try:
        d_ent = torch.from_numpy(canonical(rng, c, M * n).view(np.int64)).cuda()
        d_perm = torch.from_numpy(rng.permutation(M * n).astype(np.int64)).cuda()
        d_out = torch.empty(n * c.fr_limbs, dtype=torch.int64, device="cuda")
        beta, gamma = canonical(rng, c, 2)
        torch.cuda.synchronize()
        for name, form in (("lagrange_regular", iop.Form(iop.Lagrange, iop.Regular)), ("canonical_regular", iop.Form(iop.Canonical, iop.Regular))):
            call = lambda: iop.build_ratio_copy_constraint_device(d, d_ent.data_ptr(), [iop.Regular] * M, d_perm.data_ptr(), beta, gamma, form,
                                                                  d_out.data_ptr(), stream)
            row = {"expected_form": name, "call_ms": timed(call, reps), "stages_ms": stage_times(call, reps)}
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    finally:
        d.release()
        gm.trim(0)


if __name__ == "__main__":
    main()
