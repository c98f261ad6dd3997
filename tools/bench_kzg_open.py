"""KZG opening on one GPU: python tools/bench_kzg_open.py [out.json] (default profiles/kzg_open.json)

Per (curve, n): the divide passes alone (gmsm_poly_div_x_minus_a, device in / device out), Open end to end over a resident
key (host polynomial, as the Go method passes it, and device polynomial), and Commit of an n - 1 polynomial over the same
handle in the same process (host and device scalars); BatchOpenSinglePoint's device part at k = 8 (gmsm_poly_eval +
gmsm_kzg_open_folded over device polynomials). Host clock around blocking calls (each ends in a stream synchronise),
median of `reps` after warm-up. The divide row carries its two lower bounds: 2 reads + 1 write of n elements against
8 TB/s, and ~2n products against the measured product rate of the same limb count (profiles/peaks_r06.json). Kernel
times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
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

HBM_BYTES_PER_S = 8e12
PEAKS = json.load(open(os.path.join(ROOT, "profiles", "peaks_r06.json")))
# Fr of BN254 and BLS12-381: 8 32-bit limbs (the rate of BN254's Fp product); Fr of BW6-761: 12 (BLS12-381's Fp)
PRODUCT_RATE = {"bn254": PEAKS["bn254_fp_mul_unsigned"], "bls12_381": PEAKS["bn254_fp_mul_unsigned"],
                "bw6_761": PEAKS["bls12_381_fp_mul_unsigned"]}
ROWS = [("bn254", 16), ("bn254", 20), ("bn254", 24), ("bls12_381", 20), ("bw6_761", 20)]


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


def row(curve, logn, reps):
    c = gm.CURVES[curve]
    n = 1 << logn
    g = gm.G1Affine(curve)
    rng = np.random.default_rng([0x4B5A, logn])
    base = g.generate_points(min(n, 1 << 20), int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)))
    pts = np.ascontiguousarray(np.tile(base, (n // base.shape[0], 1)))  # timing only: repeated bases above 2^20
    rb = g.register_bases(points=pts)
    del pts
    stream = torch.cuda.current_stream().cuda_stream
    try:
        f = canonical(rng, c, n)
        point = canonical(rng, c, 1)[0]
        gamma = canonical(rng, c, 1)[0]
        d_f = torch.from_numpy(f.view(np.int64).copy()).cuda()
        d_h = torch.empty((n - 1) * c.fr_limbs, dtype=torch.int64, device="cuda")
        out = {"curve": curve, "group": "g1", "logn": logn, "n": n}
        out["divide_ms"] = timed(lambda: gm.kzg.divide_device(curve, d_f.data_ptr(), n, point, d_h.data_ptr(), stream), reps)
        out["eval_ms"] = timed(lambda: gm.kzg.poly_eval_device(curve, d_f.data_ptr(), [n], point, stream), reps)
        out["open_host_ms"] = timed(lambda: gm.kzg.Open(f, point, rb), reps)
        out["open_device_ms"] = timed(lambda: gm.kzg.open_device(d_f.data_ptr(), n, point, rb, stream), reps)
        h = f[: n - 1]
        out["commit_host_ms"] = timed(lambda: rb.MultiExp(h), reps)
        out["commit_device_ms"] = timed(lambda: rb.multiexp_device(d_f.data_ptr(), n - 1, stream), reps)
        out["open_minus_commit_host_ms"] = out["open_host_ms"] - out["commit_host_ms"]
        out["open_minus_commit_device_ms"] = out["open_device_ms"] - out["commit_device_ms"]
        elem = 8 * c.fr_limbs
        byte_ms = 3 * n * elem / HBM_BYTES_PER_S * 1e3
        prod_ms = 2 * n / PRODUCT_RATE[curve] * 1e3
        out["divide_bounds"] = {"bytes": 3 * n * elem, "byte_bound_ms": byte_ms, "products": 2 * n, "product_bound_ms": prod_ms,
                                "product_rate_per_s": PRODUCT_RATE[curve],
                                "bound_over_time": max(byte_ms, prod_ms) / out["divide_ms"],
                                "note": "divide_ms is host-timed (launches + synchronise included); kernel times: the rocprofv3 run"}
        if logn == 20:  # BatchOpenSinglePoint's device part, k = 8 polynomials of n coefficients
            k = 8
            fs = canonical(rng, c, k * n)
            d_fs = torch.from_numpy(fs.view(np.int64)).cuda()
            lens = [n] * k
            out["batch_k"] = k
            out["batch_eval_ms"] = timed(lambda: gm.kzg.poly_eval_device(curve, d_fs.data_ptr(), lens, point, stream), reps)
            out["batch_open_device_ms"] = timed(lambda: gm.kzg.batch_open_device(d_fs.data_ptr(), lens, point, gamma, rb, stream), reps)
            del d_fs
        return out
    finally:
        rb.release()
        gm.trim(0)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kzg_open.json")
    reps = int(os.environ.get("KZG_BENCH_REPS", "7"))
    rows = []
    for curve, logn in ROWS:
        r = row(curve, logn, reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    rec = {"tool": "tools/bench_kzg_open.py", "device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
