#!/usr/bin/env python3
"""Record the reference's GKR test vectors (internal/generator/gkr/test_vectors/*.json with their resources/*.json circuits:
the eight that every curve's TestGkrVectors runs) as one small data-only fixture, so that the tests need no reference tree.
Values are integers mod the scalar field (negative ones are small negatives); every challenge is the constant of "hash".

Output:  tests/golden/gkr_vectors.json
Run:     python tests/golden/make_gkr_vectors.py <gnark-crypto checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def collect(ref):
    d = os.path.join(ref, "internal", "generator", "gkr", "test_vectors")
    out = {}
    for name in sorted(os.listdir(d)):
        if not name.endswith(".json"):  # mimc_five_levels_two_instances._json is not a vector the reference runs
            continue
        with open(os.path.join(d, name)) as f:
            v = json.load(f)
        with open(os.path.join(d, v["circuit"])) as f:
            circuit = json.load(f)
        out[name[:-len(".json")]] = {
            "hash": v["hash"],
            "circuit": [[w["gate"], w["inputs"]] for w in circuit],
            "input": v["input"],
            "output": v["output"],
            "proof": [{"finalEvalProof": p["finalEvalProof"], "partialSumPolys": p["partialSumPolys"]} for p in v["proof"]],
        }
    return out


def render(vectors):
    return json.dumps(vectors, sort_keys=True, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    with open(os.path.join(HERE, "gkr_vectors.json"), "w") as f:
        f.write(render(collect(sys.argv[1])))
