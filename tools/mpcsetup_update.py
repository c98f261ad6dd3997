"""The mpcsetup point updates on one GPU: python tools/mpcsetup_update.py [out.json] (default profiles/mpcsetup_update.json).
One GPU session; run it under a time limit (timeout 600 python tools/mpcsetup_update.py).

gmsm_update_monomials and gmsm_batch_scale (per-point scalars, one scalar for all) over device-resident points and scalars:
BN254 G1 and G2 at 2^16 and 2^20, BLS12-381 G1 and BW6-761 G1 at 2^16; gmsm_linear_combinations on BN254 G1 2^20. Host
clock around blocking calls (each ends in a stream synchronise), median of `reps` after a warm-up call. Every row carries
  cpu_port_ms          the oracle's own scalar_mul loop (oracle/msm_oracle.c, a C port of the reference's windowed
                       ScalarMultiplication - NOT the Go code, and without its GLV) over 2^10 points on this machine's
                       CPU, one core, scaled to n: what the reference's one-after-another loop would take, as a port
  frac_of_measured     expected field products of the walks (per point: phi + the table's sum, one doubling per bit of
                       GLV_BITS, an addition where the digit pair is not (0, 0) - every bit for per-point scalars, where a
                       wave adds when any lane does, 3/4 of them for one scalar) x n / time / the measured product rate
                       of the coordinate field (profiles/peaks_r06.json)."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
gm = importlib.import_module("gnark-crypto_amd")

PEAKS = json.load(open(os.path.join(ROOT, "profiles", "peaks_r06.json")))
ROWS = [("bn254", "g1", 16), ("bn254", "g1", 20), ("bn254", "g2", 16), ("bn254", "g2", 20), ("bls12_381", "g1", 16), ("bw6_761", "g1", 16)]
DBL, ADD, TABLE = 9, 14, 15  # field products of double / add / phi + P1 + P2 (a product-sum counted as two), as tools/bench_to_lagrange.py
CPU_POINTS = 1 << 10


def product_rate(curve, which):
    ext2 = which == "g2" and gm.CURVES[curve].g2_ext == 2
    return PEAKS[f"{curve}_{'fp2' if ext2 else 'fp'}_mul_unsigned"]


def walk_products(curve, add_frac):
    b = gm.curves.GlvParams(gm.CURVES[curve]).bits
    return TABLE + b * DBL + b * add_frac * ADD


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


def cpu_port_ms_per_point(curve, which, pts, rng):
    import oracle
    o = oracle.Oracle(curve, which)
    r = gm.CURVES[curve].r
    ks = [int.from_bytes(rng.bytes(64), "little") % r for _ in range(CPU_POINTS)]
    t0 = time.perf_counter()
    for i in range(CPU_POINTS):
        o.scalar_mul(pts[i], ks[i])
    return (time.perf_counter() - t0) * 1e3 / CPU_POINTS


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mpcsetup_update.json")
    reps = int(os.environ.get("MPCSETUP_BENCH_REPS", "5"))
    stream = torch.cuda.current_stream().cuda_stream
    out = {"tool": "tools/mpcsetup_update.py", "device": torch.cuda.get_device_name(0), "reps": reps, "cpu_port_points": CPU_POINTS,
           "cpu_port": "oracle scalar_mul (C port of the reference's windowed ScalarMultiplication, no GLV), one core, scaled to n", "rows": []}
    m = gm.mpcsetup
    try:
        for curve, which, logn in ROWS:
            c = gm.CURVES[curve]
            n = 1 << logn
            g = (gm.G1Affine if which == "g1" else gm.G2Affine)(curve)
            rng = np.random.default_rng([0x3C9, logn, ROWS.index((curve, which, logn))])
            pts = g.generate_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)))
            d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
            d_out = torch.empty_like(d_pts)
            d_sc = torch.from_numpy(canonical(rng, c, n).view(np.int64)).cuda()
            r = canonical(rng, c, 1)[0]
            row = {"curve": curve, "group": which, "logn": logn}
            row["update_monomials_ms"] = timed(lambda: m.update_monomials_device(curve, which, d_pts.data_ptr(), n, r, d_out.data_ptr(), stream), reps)
            row["batch_scale_ms"] = timed(lambda: m.batch_scale_device(curve, which, d_pts.data_ptr(), n, d_sc.data_ptr(), n, d_out.data_ptr(), stream), reps)
            row["scale_one_ms"] = timed(lambda: m.batch_scale_device(curve, which, d_pts.data_ptr(), n, d_sc.data_ptr(), 1, d_out.data_ptr(), stream), reps)
            rate = product_rate(curve, which)
            row["product_rate_per_s"] = rate
            row["frac_of_measured"] = {k: walk_products(curve, f) * n / rate * 1e3 / row[k + "_ms"]
                                       for k, f in (("update_monomials", 1.0), ("batch_scale", 1.0), ("scale_one", 0.75))}
            per_point = cpu_port_ms_per_point(curve, which, pts, rng)
            row["cpu_port_ms"] = per_point * n
            row["cpu_port_over_update_monomials"] = row["cpu_port_ms"] / row["update_monomials_ms"]
            if (curve, which, logn) == ("bn254", "g1", 20):
                ends = [n // 4, n // 2, n]
                row["linear_combinations_ms"] = timed(lambda: m.linear_combinations_device(curve, which, d_pts.data_ptr(), n, r, ends, stream), reps)
                row["multiexp_ms"] = timed(lambda: g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream), reps)
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
            del d_pts, d_out, d_sc
            with open(path, "w") as f:
                json.dump(out, f, indent=1)
    finally:
        gm.trim(0)


if __name__ == "__main__":
    main()
