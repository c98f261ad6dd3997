"""shplonk.BatchOpen on one GPU: python tools/shplonk_open.py [out.json] (default profiles/shplonk_open.json). One GPU
session; run it under a time limit (timeout 300 python tools/shplonk_open.py).

BN254, k = 4 polynomials of 2^20 coefficients, two points each, device-resident inputs: the time of open_w (8 divisions,
the accumulation, Commit(w)) and of open_wprime (the combination, one division, Commit(w')), and from the same process
and handle one Commit of 2^20 device scalars and one gmsm_poly_div_x_minus_a of 2^20 (device in / device out). Host clock
around blocking calls (each ends in a stream synchronise), median of `reps` after a warm-up call. The two ratios DESIGN
states: open_w / (sum m_i divisions + one commit) and open_wprime / (one division + one commit)."""
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

CURVE, LOGN, K, M = "bn254", 20, 4, 2


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


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shplonk_open.json")
    reps = int(os.environ.get("SHPLONK_BENCH_REPS", "7"))
    c = gm.CURVES[CURVE]
    n = 1 << LOGN
    g = gm.G1Affine(CURVE)
    rng = np.random.default_rng([0x5B2A, LOGN])
    base = g.generate_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)))
    size = n + K * M  # the reference's size condition asks for n + K M - 1 bases; timing only: the first ones repeat
    rb = g.register_bases(points=np.ascontiguousarray(np.concatenate([base, base[:K * M]])))
    del base
    stream = torch.cuda.current_stream().cuda_stream
    try:
        lens = [n] * K
        d_polys = torch.from_numpy(canonical(rng, c, K * n).view(np.int64)).cuda()
        points = [canonical(rng, c, M) for _ in range(K)]
        gamma, z, a = canonical(rng, c, 3)
        d_w = torch.empty(n * c.fr_limbs, dtype=torch.int64, device="cuda")
        d_h = torch.empty((n - 1) * c.fr_limbs, dtype=torch.int64, device="cuda")
        out = {"tool": "tools/shplonk_open.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE, "group": "g1",
               "logn": LOGN, "k": K, "points_per_polynomial": M, "registered_bases": size}
        claimed, _ = gm.shplonk.open_w_device(d_polys.data_ptr(), lens, points, gamma, rb, d_w.data_ptr(), stream)
        out["open_w_ms"] = timed(lambda: gm.shplonk.open_w_device(d_polys.data_ptr(), lens, points, gamma, rb, d_w.data_ptr(), stream), reps)
        out["open_wprime_ms"] = timed(lambda: gm.shplonk.open_wprime_device(d_polys.data_ptr(), lens, points, claimed, gamma, d_w.data_ptr(),
                                                                           z, rb, stream), reps)
        out["commit_ms"] = timed(lambda: rb.multiexp_device(d_polys.data_ptr(), n, stream), reps)
        out["divide_ms"] = timed(lambda: gm.kzg.divide_device(CURVE, d_polys.data_ptr(), n, a, d_h.data_ptr(), stream), reps)
        out["open_w_over_divisions_plus_commit"] = out["open_w_ms"] / (K * M * out["divide_ms"] + out["commit_ms"])
        out["open_wprime_over_division_plus_commit"] = out["open_wprime_ms"] / (out["divide_ms"] + out["commit_ms"])
        print(json.dumps(out), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    finally:
        rb.release()
        gm.trim(0)


if __name__ == "__main__":
    main()
