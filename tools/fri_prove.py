"""fr/fri's prover on one GPU: python tools/fri_prove.py [out.json] (default profiles/fri_prove.json).
One GPU session; run it under a time limit (timeout 300 python tools/fri_prove.py).

BN254, p resident on the device, sizes 2^13 and 2^17 (N = 2^16 and 2^20). Each row is the host clock around the blocking calls,
median of `reps` after a warm-up call:
  commit       gmsm_fri_commit: the transform, the gather into the sorted layer, tree 0
  fold_first   gmsm_fri_fold of layer 0: N -> N/2 elements and the tree over them
  fold_last    the last fold that builds a tree (32 -> 16 elements); the fold after it (16 -> 8) leaves the Evaluation alone
  query        gmsm_fri_query of all nbSteps steps, copied back to the host
  prove        fri.BuildProofOfProximity(d_p): a commit, nbSteps folds, one query and the transcript between them
  open         fri.Open(oracle, position) from the oracle a proof has folded: one gather
  transcript   the host time of the proof's transcript alone: nbSteps + 1 challenges over mimc.NewMiMC and the query positions
What the times stand against, from the same run: the parent commit's own pieces for the same shapes - gmsm_fft (DIF) over N
device-resident elements plus gmsm_merkle_new over d_leaves for N, N/2, ..., 16 leaves without keeping them - which is what a
prover built from those entries alone would launch, before the copies of every folded layer to the host and back that it would
also need. No threshold is set. There is no Go toolchain here, so no reference time stands next to these. No ratio is claimed."""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gm = importlib.import_module("gnark-crypto_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from iop_expr import canonical, timed  # noqa: E402

CURVE = "bn254"


def timed_once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def pieces(c, dom, data, N, stream, reps):
    """(gmsm_fft over N, [gmsm_merkle_new over N, N/2, ..., 16 leaves]) in ms"""
    work = data[:N * c.fr_limbs].clone()
    fft_ms = timed(lambda: dom.fft_device(work.data_ptr(), gm.fft.DIF, stream=stream), reps)
    trees_ms = []
    n = N
    while n >= 16:
        def build(n=n):
            gm.merkletree.DeviceTree(c, d_leaves=data.data_ptr(), n=n, leaf_len=1, keep_leaves=False, stream=stream).Release()
        trees_ms.append(timed(build, reps))
        n //= 2
    return fft_ms, trees_ms


def folded(s, d_p, size, stream, upto):
    """an oracle folded `upto` times with fixed challenges"""
    c = s.curve
    o = s.Commit(d_p=d_p, n=size, stream=stream)
    for k in range(upto):
        o.fold(gm.polynomial.from_int(c, 0x1234567 + k))
    return o


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fri_prove.json")
    reps = int(os.environ.get("FRI_PROVE_REPS", "7"))
    c = gm.CURVES[CURVE]
    rng = np.random.default_rng([0xF21, 1])
    out = {"tool": "tools/fri_prove.py", "device": torch.cuda.get_device_name(0), "reps": reps, "curve": CURVE, "rows": []}
    stream = torch.cuda.current_stream().cuda_stream
    data = torch.from_numpy(canonical(rng, c, 1 << 20).view(np.int64).reshape(-1)).cuda()
    torch.cuda.synchronize()
    for logsize in (13, 17):
        size = 1 << logsize
        s = gm.fri.RADIX_2_FRI.New(CURVE, size, gm.mimc.Factory(CURVE))
        N, steps = s.Cardinality, s.nbSteps
        dom = s._device_domain()
        fft_ms, trees_ms = pieces(c, dom, data, N, stream, reps)
        row = {"size": size, "cardinality": N, "nb_steps": steps, "pieces_fft_ms": fft_ms, "pieces_trees_ms": trees_ms,
               "pieces_sum_ms": fft_ms + sum(trees_ms[:steps])}
        d_p = data.data_ptr()
        row["commit_ms"] = timed(lambda: s.Commit(d_p=d_p, n=size, stream=stream).Release(), reps)
        row["commit_pieces_ms"] = fft_ms + trees_ms[0]

        def fold_at(k):  # a fold consumes its oracle: a fresh one, folded k times, for every repetition; the first is the warm-up
            ts = []
            for _ in range(reps + 1):
                o = folded(s, d_p, size, stream, k)
                torch.cuda.synchronize()
                ts.append(timed_once(lambda: o.fold(gm.polynomial.from_int(c, 77))))
                o.Release()
            return float(np.median(ts[1:]))
        row["fold_first_ms"], row["fold_first_pieces_ms"] = fold_at(0), trees_ms[1]
        row["fold_last_ms"], row["fold_last_pieces_ms"] = fold_at(steps - 2), trees_ms[steps - 1]
        o = folded(s, d_p, size, stream, steps)
        positions = gm.fri.deriveQueriesPositions(12345 % N, N, steps)
        row["query_ms"] = timed(lambda: o.query_limbs(positions), reps)
        row["open_ms"] = timed(lambda: s.Open(o, 4321 % N), reps)
        o.Release()
        proofs = []
        row["prove_ms"] = timed(lambda: proofs.append(s.BuildProofOfProximity(d_p=d_p, n=size, stream=stream)), reps)
        s.VerifyProofOfProximity(proofs[-1])
        rnd = proofs[-1].Rounds[0]

        def transcript():
            xis, fs = s._transcript()
            fs.Bind(xis[0], bytes(32))
            for i in range(steps):
                fs.Bind(xis[i], rnd.Interactions[i][0].MerkleRoot)
                fs.ComputeChallenge(xis[i])
            s._positions(fs, xis, rnd.Evaluation)
        row["transcript_ms"] = timed(transcript, reps)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
        s.Release()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    gm.trim(0)


if __name__ == "__main__":
    main()
