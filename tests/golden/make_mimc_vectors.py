#!/usr/bin/env python3
"""Record the reference's MiMC test vectors for BN254 (ecc/bn254/fr/mimc/test_vectors/vectors.json: ten messages of one to
five elements with their digests, hex integers) as a small data-only fixture, so that the tests need no reference tree.

Output:  tests/golden/mimc_vectors.json
Run:     python tests/golden/make_mimc_vectors.py <gnark-crypto checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def collect(ref):
    with open(os.path.join(ref, "ecc", "bn254", "fr", "mimc", "test_vectors", "vectors.json")) as f:
        vectors = json.load(f)
    return {"bn254": [{"in": v["in"], "out": v["out"]} for v in vectors]}


def render(vectors):
    return json.dumps(vectors, sort_keys=True, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    with open(os.path.join(HERE, "mimc_vectors.json"), "w") as f:
        f.write(render(collect(sys.argv[1])))
