"""fflonk.BatchOpen on one GPU: python tools/fflonk_open.py [out.json] (default profiles/fflonk_open.json). One GPU
session; run it under a time limit (timeout 300 python tools/fflonk_open.py).

BN254, one pack of 8 polynomials of 2^17 coefficients (t = 8, folded length 2^20) opened at 2 base points, device-resident
inputs. Two rows, three medians each (every median over `reps` calls after a warm-up call, host clock around blocking
calls - each ends in a stream synchronise):
  fflonk    gmsm_fflonk_open_w / gmsm_fflonk_open_wprime: 8 chains of 2 scans over 2^17 coefficients
  baseline  the same opening by gmsm_fflonk_fold + gmsm_shplonk_open_w / _wprime over the extended sets: one chain of 16
            scans over 2^20 coefficients
and, from the same process and handle, the stages both rows are made of: one Commit of 2^20 device scalars, one division
of 2^17 and one of 2^20 (gmsm_poly_div_x_minus_a, device in / device out), the fold, FoldAndCommit. The part of open_w that
is not its commitment is reported for both rows, and the ratio of the two: the scan work falls by t."""
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

CURVE, LOGN, PACK, M = "bn254", 17, 8, 2


def canonical(rng, c, n):
    a = rng.integers(0, 2**64, size=(n, c.fr_limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (c.fr_bits - 64 * (c.fr_limbs - 1) - 1)) - 1)
    return a


def timed(fn, reps):
    """three medians of `reps` calls each, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    medians = []
    for _ in range(3):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        medians.append(statistics.median(ts))
    return medians


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fflonk_open.json")
    reps = int(os.environ.get("FFLONK_BENCH_REPS", "7"))
    c = gm.CURVES[CURVE]
    n = 1 << LOGN
    t = gm.fflonk.NextDivisor(CURVE, PACK)
    folded = t * n
    g = gm.G1Affine(CURVE)
    rng = np.random.default_rng([0xFF2A, LOGN])
    base = g.generate_points(folded, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)))
    size = folded + t * M  # the size condition asks for folded + t M - 1 bases; timing only: the first ones repeat
    rb = g.register_bases(points=np.ascontiguousarray(np.concatenate([base, base[:t * M]])))
    del base
    stream = torch.cuda.current_stream().cuda_stream
    try:
        lens = [n] * PACK
        d_polys = torch.from_numpy(canonical(rng, c, PACK * n).view(np.int64)).cuda()
        points = [canonical(rng, c, M)]
        gamma, z, a = canonical(rng, c, 3)
        d_w = torch.empty(folded * c.fr_limbs, dtype=torch.int64, device="cuda")
        d_w2 = torch.empty(folded * c.fr_limbs, dtype=torch.int64, device="cuda")
        d_f = torch.empty(folded * c.fr_limbs, dtype=torch.int64, device="cuda")
        d_h = torch.empty((folded - 1) * c.fr_limbs, dtype=torch.int64, device="cuda")
        out = {"tool": "tools/fflonk_open.py", "device": torch.cuda.get_device_name(0), "reps": reps, "medians_per_row": 3, "curve": CURVE,
               "group": "g1", "pack": PACK, "t": t, "logn": LOGN, "folded_len": folded, "base_points": M, "registered_bases": size}
        # row 1: the new entries
        _, fclaimed, W = gm.fflonk.open_w_device(d_polys.data_ptr(), lens, [PACK], points, gamma, rb, d_w.data_ptr(), stream)
        row = {"open_w_ms": timed(lambda: gm.fflonk.open_w_device(d_polys.data_ptr(), lens, [PACK], points, gamma, rb, d_w.data_ptr(), stream), reps),
               "open_wprime_ms": timed(lambda: gm.fflonk.open_wprime_device(d_polys.data_ptr(), lens, [PACK], points, fclaimed, gamma,
                                                                           d_w.data_ptr(), z, rb, stream), reps)}
        out["fflonk"] = row
        # row 2: fold, then shplonk over the folded polynomial and the extended set
        pts = [int.from_bytes(p.astype("<u8").tobytes(), "little") * pow(c.fr_R, -1, c.r) % c.r for p in points[0]]
        omega = pow(c.fr_mult_gen, (c.r - 1) // t, c.r)
        ext_true = [x * pow(omega, l, c.r) % c.r for x in pts for l in range(t)]
        ext = [np.array([[(v * c.fr_R % c.r >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(c.fr_limbs)] for v in ext_true], dtype=np.uint64)]
        gm.fflonk.fold_device(CURVE, d_polys.data_ptr(), lens, d_f.data_ptr(), stream)
        sclaimed, sW = gm.shplonk.open_w_device(d_f.data_ptr(), [folded], ext, gamma, rb, d_w2.data_ptr(), stream)
        out["same_W"] = bool((sW == W).all())
        out["same_w"] = bool(torch.equal(d_w, d_w2))
        out["same_inner_claimed"] = bool((sclaimed[0] == fclaimed[0]).all())
        base_row = {"fold_ms": timed(lambda: gm.fflonk.fold_device(CURVE, d_polys.data_ptr(), lens, d_f.data_ptr(), stream), reps),
                    "open_w_ms": timed(lambda: gm.shplonk.open_w_device(d_f.data_ptr(), [folded], ext, gamma, rb, d_w2.data_ptr(), stream), reps),
                    "open_wprime_ms": timed(lambda: gm.shplonk.open_wprime_device(d_f.data_ptr(), [folded], ext, sclaimed, gamma, d_w2.data_ptr(),
                                                                                 z, rb, stream), reps)}
        out["baseline"] = base_row
        # the stages
        out["commit_folded_ms"] = timed(lambda: rb.multiexp_device(d_f.data_ptr(), folded, stream), reps)
        out["fold_commit_ms"] = timed(lambda: gm.fflonk.fold_commit_device(d_polys.data_ptr(), lens, rb, None, stream), reps)
        out["divide_member_ms"] = timed(lambda: gm.kzg.divide_device(CURVE, d_polys.data_ptr(), n, a, d_h.data_ptr(), stream), reps)
        out["divide_folded_ms"] = timed(lambda: gm.kzg.divide_device(CURVE, d_f.data_ptr(), folded, a, d_h.data_ptr(), stream), reps)
        med = statistics.median
        commit = med(out["commit_folded_ms"])
        out["fflonk_open_w_minus_commit_ms"] = med(row["open_w_ms"]) - commit
        out["baseline_open_w_minus_commit_ms"] = med(base_row["open_w_ms"]) - commit
        out["scan_part_ratio_baseline_over_fflonk"] = out["baseline_open_w_minus_commit_ms"] / out["fflonk_open_w_minus_commit_ms"]
        out["open_w_ratio_baseline_over_fflonk"] = (med(base_row["fold_ms"]) + med(base_row["open_w_ms"])) / med(row["open_w_ms"])
        out["open_wprime_ratio_baseline_over_fflonk"] = med(base_row["open_wprime_ms"]) / med(row["open_wprime_ms"])
        print(json.dumps(out), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    finally:
        rb.release()
        gm.trim(0)


if __name__ == "__main__":
    main()
