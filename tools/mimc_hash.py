"""MiMC batches and Merkle trees on one GPU: python tools/mimc_hash.py [out.json] (default profiles/mimc_hash.json).
One GPU session; run it under a time limit (timeout 300 python tools/mimc_hash.py).

BN254, device-resident inputs. Each row is the host clock around the blocking call (it ends in a stream synchronise), median of
`reps` after a warm-up call:
  batch   gmsm_mimc_sum_batch of 2^20 messages of 1 and of 2 blocks
  tree    gmsm_merkle_new over 2^16 and 2^20 single-element leaves (the leaves kept: a device-to-device copy is part of it)
  prove   gmsm_merkle_prove of 1024 paths of the 2^20 tree, leaves included, copied back to the host
Beside each hashing time a floor from a number that does not come from the code under test: its fr products, 3 per round and
block (110 rounds), at a product rate measured in the same run - a straight-line program of 64 dependent products per index
over 2^20 indices through gmsm_iop_evaluate_expression (kernel time, stage slot 0), as tools/iop_expr.py measures its kernels.
That program pays the interpreter's register traffic, so the rate is what this library reaches elsewhere, not the chip's peak;
the rate of profiles/peaks_r06.json (bn254_fp_mul, a bare product loop) and its floor stand next to it.
No threshold is set. There is no Go toolchain here, so no reference time stands next to these. No ratio is claimed."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from iop_expr import canonical, kernel_ms, product_rate, timed  # noqa: E402

CURVE, ROUNDS, CHAIN = "bn254", 110, 64


def chain(i, x):
    y = x
    for _ in range(CHAIN):
        y = y * x
    return y


def measured_product_rate(c, rng, reps):
    n = 1 << 20
    iop = gm.iop
    x = torch.from_numpy(canonical(rng, c, n).view(np.int64).reshape(-1)).cuda()
    out = torch.empty_like(x)
    code = iop.trace(CURVE, chain, 1)
    assert [int(w) & 0xFF for w in code.words].count(iop.EXPR_MUL) == CHAIN
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: iop.evaluate_expression_device(CURVE, code, [x.data_ptr()], n, [n], [0], [iop.Regular], iop.Regular, out.data_ptr(), stream=stream)
    call()
    torch.cuda.synchronize()
    return CHAIN * n / (kernel_ms(call, reps) * 1e-3)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mimc_hash.json")
    reps = int(os.environ.get("MIMC_HASH_REPS", "7"))
    c = gm.CURVES[CURVE]
    rng = np.random.default_rng([0x313C, 1])
    rate, peak = measured_product_rate(c, rng, reps), product_rate()
    out = {"tool": "tools/mimc_hash.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE, "rounds": ROUNDS,
           "product_rate_per_s": rate, "product_rate_source": "same run: %d dependent products per index, 2^20 indices, gmsm_iop_evaluate_expression kernel time" % CHAIN,
           "peak_product_rate_per_s": peak, "peak_product_rate_source": "profiles/peaks_r06.json bn254_fp_mul", "rows": []}

    def add(row, blocks=None):
        if blocks is not None:
            row["products"] = 3 * ROUNDS * blocks
            row["floor_products_ms"] = row["products"] / rate * 1e3
            if peak:
                row["floor_peak_products_ms"] = row["products"] / peak * 1e3
        out["rows"].append(row)
        print(json.dumps(row), flush=True)

    stream = torch.cuda.current_stream().cuda_stream
    n = 1 << 20
    data = torch.from_numpy(canonical(rng, c, 2 * n).view(np.int64).reshape(-1)).cuda()
    digests = torch.empty(n * c.fr_limbs, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for blocks in (1, 2):
        call = lambda: gm.mimc.sum_batch_device(c, data.data_ptr(), n, blocks, blocks, digests.data_ptr(), stream=stream)
        add({"what": "batch", "count": n, "blocks": blocks, "call_ms": timed(call, reps)}, n * blocks)
    big = None
    for logn in (16, 20):
        m = 1 << logn
        trees = []

        def build():
            trees.append(gm.merkletree.DeviceTree(c, d_leaves=data.data_ptr(), n=m, leaf_len=1, keep_leaves=True, stream=stream))
            if len(trees) > 1:
                trees.pop(0).Release()
        add({"what": "tree", "leaves": m, "leaf_len": 1, "depth": logn, "call_ms": timed(build, reps)}, m + 2 * (m - 1))
        if logn == 20:
            big = trees.pop()
        for t in trees:
            t.Release()
    idx = rng.integers(0, big.n, size=1024, dtype=np.uint64)
    add({"what": "prove", "leaves": big.n, "paths": len(idx), "call_ms": timed(lambda: big.prove_limbs(idx), reps)})
    big.Release()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    gm.trim(0)


if __name__ == "__main__":
    main()
