"""iop.Polynomial on one GPU: python tools/iop_poly.py [out.json] (default profiles/iop_poly.json).
One GPU session; run it under a time limit (timeout 300 python tools/iop_poly.py).

BN254, a polynomial of size n = 2^20 and the big domain N = 2^22, everything device-resident. Each row is the host clock around
the blocking call (it ends in a stream synchronise), median of `reps` after a warm-up call:
  to_basis_*            gmsm_iop_to_basis: Canonical -> Lagrange on n (one transform), Canonical -> LagrangeCoset on N with
                        len = n (the zero-fill and one coset transform), Lagrange -> LagrangeCoset on n (two transforms)
  evaluate_lagrange_k1, _k8   gmsm_iop_evaluate in Lagrange basis at a random x, len = n; beside them batch_invert_n,
                        gmsm_fr_batch_invert of the same n: the inversion the reference's evalLagrange starts with
  evaluate_canonical_k1 gmsm_iop_evaluate in Canonical basis, len = n
  divide_by_x_minus_one gmsm_iop_divide_by_x_minus_one over (n, N); beside it, from the same run, fft_inverse_coset_N: one
                        inverse coset gmsm_fft of the same N, the floor the quotient sits on
`estimate` holds the rough product count of the barycentric kernel, (5 + k) field products per coefficient, against the
measured product rate of profiles/peaks_r06.json when that file has one: something to check against, not a threshold.
There is no Go toolchain here, so no reference time stands next to these. No ratio is claimed."""
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

CURVE, LOGN, LOGBIG = "bn254", 20, 22


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


def product_rate():
    """products per second of a 254-bit field on one MI355X (profiles/peaks_r06.json: BN254's coordinate field, which has the
    limb count of its scalar field), or None"""
    try:
        return float(json.load(open(os.path.join(ROOT, "profiles", "peaks_r06.json")))["bn254_fp_mul"])
    except (OSError, KeyError, ValueError):
        return None


def estimate(n):
    rate = product_rate()
    est = {"products_per_coefficient": "5 + k", "products_k1": 6 * n, "products_k8": 13 * n, "product_rate_per_s": rate,
           "source": "profiles/peaks_r06.json bn254_fp_mul"}
    if rate:
        est["floor_ms_k1"], est["floor_ms_k8"] = 6 * n / rate * 1e3, 13 * n / rate * 1e3
    return est


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "iop_poly.json")
    reps = int(os.environ.get("IOP_POLY_REPS", "7"))
    c = gm.CURVES[CURVE]
    n, big = 1 << LOGN, 1 << LOGBIG
    rng = np.random.default_rng([0x10C, LOGN])
    stream = torch.cuda.current_stream().cuda_stream
    iop = gm.iop
    out = {"tool": "tools/iop_poly.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE, "logn": LOGN, "log_big": LOGBIG,
           "estimate": estimate(n), "rows": []}
    ds, db = gm.fft.NewDomain(CURVE, n), gm.fft.NewDomain(CURVE, big)
    try:
        d_n = torch.from_numpy(canonical(rng, c, 8 * n).view(np.int64)).cuda()        # 8 polynomials of n coefficients
        d_big = torch.from_numpy(canonical(rng, c, big).view(np.int64)).cuda()
        d_out = torch.empty(big * c.fr_limbs, dtype=torch.int64, device="cuda")
        x, g = canonical(rng, c, 2)
        torch.cuda.synchronize()
        can, lag, cos = (iop.Form(b, iop.Regular) for b in (iop.Canonical, iop.Lagrange, iop.LagrangeCoset))
        rows = [
            # the transforms run on whatever the buffer holds: a time does not depend on the values
            ("to_basis_canonical_to_lagrange_n", lambda: iop.to_basis_device(ds, d_n.data_ptr(), n, can, iop.Lagrange, stream)),
            ("to_basis_canonical_to_lagrange_coset_N_len_n", lambda: iop.to_basis_device(db, d_out.data_ptr(), n, can, iop.LagrangeCoset, stream)),
            ("to_basis_lagrange_to_lagrange_coset_n", lambda: iop.to_basis_device(ds, d_n.data_ptr(), n, lag, iop.LagrangeCoset, stream)),
            ("evaluate_lagrange_k1", lambda: iop.evaluate_device(CURVE, d_n.data_ptr(), 1, n, n, iop.Lagrange, [iop.Regular], 0, None, x, stream)),
            ("evaluate_lagrange_k8", lambda: iop.evaluate_device(CURVE, d_n.data_ptr(), 8, n, n, iop.Lagrange, [iop.Regular] * 8, 0, None, x, stream)),
            ("batch_invert_n", lambda: iop.batch_invert_device(CURVE, d_n.data_ptr(), n, d_out.data_ptr(), stream)),
            ("evaluate_canonical_k1", lambda: iop.evaluate_device(CURVE, d_n.data_ptr(), 1, n, n, iop.Canonical, [iop.Regular], 0, None, x, stream)),
            ("divide_by_x_minus_one", lambda: iop.divide_by_x_minus_one_device((ds, db), d_big.data_ptr(), cos, 0, d_out.data_ptr(), stream)),
            ("fft_inverse_coset_N", lambda: db.fft_device(d_out.data_ptr(), gm.fft.DIT, gm.fft.OnCoset(), inverse=True, stream=stream)),
        ]
        for name, call in rows:
            row = {"what": name, "call_ms": timed(call, reps)}
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    finally:
        ds.release()
        db.release()
        gm.trim(0)


if __name__ == "__main__":
    main()
