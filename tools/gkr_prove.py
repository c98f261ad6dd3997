"""GKR sumcheck rounds and a whole gkr.Prove on one GPU: python tools/gkr_prove.py [--hash sha256|mimc] [out.json] (default
profiles/gkr_prove.json).
One GPU session; run it under a time limit (timeout 300 python tools/gkr_prove.py).

BN254, device-resident assignments. Each row is the host clock around the blocking calls (each ends in a stream synchronise),
median of `reps` after a warm-up:
  claim_new / first_next   the first round (gmsm_gkr_claim_new: copies of the tables, the eq table, the round polynomial) and
                           the first gmsm_gkr_claim_next (fold + round polynomial in one pass) of the MiMC gate (x + y)^7, 2
                           inputs, declared degree 7, one evaluation point, at 2^17 and 2^20 instances
  eq                       gmsm_multilin_eq at n = 20
  prove                    gkr.Prove of the reference benchmark's shape, mimcCircuit(91) (gkr_test.go:314-324, 445-475) at 2^17
                           instances, over a sha256 transcript or, with --hash mimc, over mimc.NewMiMC as the reference's
                           benchmark hashes (the transcript is host work either way: a few blocks per challenge through
                           gmsm_mimc_hash); and WireAssignment.Complete before it
Beside each round two floors from numbers that do not come from the code under test:
  floor_copy_ms      the bytes it must move at the rate of a device-to-device copy measured in the same run (read plus write):
                     claim_new reads and writes the m tables, writes E and reads all m + 1; next reads m + 1 tables and writes
                     their halves
  floor_products_ms  its products at the measured rate of profiles/peaks_r06.json (bn254_fp_mul): claim_new one per element of
                     E and (gate products + 1) (degree + 1) per pair; next two per quarter and table for the fold, then the same
No threshold is set. There is no Go toolchain here, so no reference time stands next to these. No ratio is claimed."""
import hashlib
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

CURVE = "bn254"


def mimc(x, y):
    s = x + y
    s3 = s * s * s
    return s3 * s3 * s


def canonical(rng, c, n):
    a = rng.integers(0, 2**64, size=(n, c.fr_limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (c.fr_bits - 64 * (c.fr_limbs - 1) - 1)) - 1)
    return a


def median_ms(samples):
    return statistics.median(samples) * 1e3


def product_rate():
    try:
        return float(json.load(open(os.path.join(ROOT, "profiles", "peaks_r06.json")))["bn254_fp_mul"])
    except (OSError, KeyError, ValueError):
        return None


def main():
    argv = sys.argv[1:]
    hash_name = "sha256"
    if "--hash" in argv:
        at = argv.index("--hash")
        hash_name = argv[at + 1]
        del argv[at:at + 2]
    if hash_name not in ("sha256", "mimc"):
        sys.exit("--hash takes sha256 or mimc")
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "gkr_prove.json")
    reps = int(os.environ.get("GKR_PROVE_REPS", "7"))
    c = gm.CURVES[CURVE]
    rng = np.random.default_rng([0x6B, 1])
    gate = gm.gkr.Gate(mimc, 7)
    m, degree = 2, 7
    products = [int(w) & 0xFF for w in gate.code(c, m).words].count(gm.iop.EXPR_MUL)
    rate = product_rate()
    out = {"tool": "tools/gkr_prove.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE,
           "product_rate_per_s": rate, "product_rate_source": "profiles/peaks_r06.json bn254_fp_mul", "rows": []}
    for logn in (17, 20):
        n = 1 << logn
        tables = [torch.from_numpy(canonical(rng, c, n).view(np.int64).reshape(-1)).cuda() for _ in range(m)]
        scratch = torch.empty_like(tables[0])
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            scratch.copy_(tables[0])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        bytes_table = n * c.fr_limbs * 8
        copy_rate = 2 * bytes_table / statistics.median(ts[1:])
        point, r = canonical(rng, c, logn), canonical(rng, c, 1)[0]
        t_new, t_next = [], []
        for _ in range(reps + 1):
            claim = gm.gkr.Claim(c, gate, [t.data_ptr() for t in tables], n, [point], device=True)
            t0 = time.perf_counter()
            claim.Combine(r)
            t1 = time.perf_counter()
            claim.Next(r)
            t2 = time.perf_counter()
            claim.release()
            t_new.append(t1 - t0)
            t_next.append(t2 - t1)
        per_pair = (products + 1) * (degree + 1)
        rows = [{"what": "claim_new", "logn": logn, "call_ms": median_ms(t_new[1:]), "floor_copy_ms": (3 * m + 2) * bytes_table / copy_rate * 1e3,
                 "products": n + per_pair * (n // 2)},
                {"what": "first_next", "logn": logn, "call_ms": median_ms(t_next[1:]), "floor_copy_ms": 1.5 * (m + 1) * bytes_table / copy_rate * 1e3,
                 "products": 2 * (m + 1) * (n // 4) + per_pair * (n // 4)}]
        for row in rows:
            row["copy_bytes_per_s"] = copy_rate
            if rate:
                row["floor_products_ms"] = row["products"] / rate * 1e3
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        del tables, scratch
    # gmsm_multilin_eq at n = 20
    n = 20
    q, scale = canonical(rng, c, n), canonical(rng, c, 1)[0]
    d_out = torch.empty((1 << n) * c.fr_limbs, dtype=torch.int64, device="cuda")
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        gm.polynomial.eq_device(c, q, scale, d_out.data_ptr())
        ts.append(time.perf_counter() - t0)
    row = {"what": "eq", "logn": n, "call_ms": median_ms(ts[1:])}
    out["rows"].append(row)
    print(json.dumps(row), flush=True)
    del d_out
    # the reference benchmark's shape: mimcCircuit(91) at 2^17 instances
    K = gm.gkr
    rounds, n = 91, 1 << 17
    circuit = K.Circuit(K.Wire() for _ in range(rounds + 2))
    for i in range(2, len(circuit)):
        circuit[i].Gate, circuit[i].Inputs = gate, [circuit[i - 1], circuit[0]]
    ins = [torch.from_numpy(canonical(rng, c, n).view(np.int64).reshape(-1)).cuda() for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = K.WireAssignment(c, {circuit[0]: ins[0].data_ptr(), circuit[1]: ins[1].data_ptr()}, nb_instances=n, device=True).Complete(circuit)
    t1 = time.perf_counter()
    proof = K.Prove(circuit, a, gm.fiatshamir.WithHash(hashlib.sha256 if hash_name == "sha256" else gm.mimc.Factory(CURVE)))
    t2 = time.perf_counter()
    row = {"what": "prove", "circuit": "mimcCircuit(91)", "logn": 17, "transcript": hash_name, "complete_ms": (t1 - t0) * 1e3,
           "prove_ms": (t2 - t1) * 1e3, "runs": 1, "proof_elements": sum(sum(len(p) for p in w.PartialSumPolys) + len(w.FinalEvalProof) for w in proof)}
    out["rows"].append(row)
    print(json.dumps(row), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    gm.trim(0)


if __name__ == "__main__":
    main()
