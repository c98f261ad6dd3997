"""tests/mimc_model.py against what is known of the reference without running it: Keccak-256's empty-string digest, the ten
BN254 vectors of ecc/bn254/fr/mimc/test_vectors (tests/golden/mimc_vectors.json), the constants' counts; and the tree: the
level-by-level form the device builds equals the restated subtree-stack algorithm of tree.go - root and proof set of every
index for n = 1..40 - and verify.go's verifier accepts exactly those proofs."""
import hashlib
import importlib
import json
import os

import pytest

import mimc_model as mm

curves = importlib.import_module("gnark-crypto_amd.curves")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "mimc_vectors.json")) as f:
        return json.load(f)["bn254"]


def sha_H(*data):
    return hashlib.sha256(b"".join(data)).digest()


def test_keccak256_of_the_empty_string():
    assert mm.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert mm.keccak256(b"") != hashlib.sha3_256(b"").digest()  # the legacy padding, not SHA-3's
    # two blocks: the absorb loop, and a message that ends one byte short of the rate (padding 0x81 in one byte)
    assert mm.keccak256(b"a" * 135) != mm.keccak256(b"a" * 136) and len(mm.keccak256(b"a" * 300)) == 32


def test_the_reference_vectors_reproduce():
    vs = vectors()
    assert len(vs) == 10 and {len(v["in"]) for v in vs} == {1, 2, 3, 4, 5}
    for v in vs:
        assert mm.mimc(curves.BN254, [int(x, 16) for x in v["in"]]) == int(v["out"], 16)


def test_constant_counts_and_ranges():
    for name, rounds in (("bn254", 110), ("bls12_381", 111), ("bw6_761", 163)):
        c = curves.CURVES[name]
        cs = mm.constants(c)
        assert len(cs) == rounds and all(0 <= v < c.r for v in cs) and len(set(cs)) == rounds
    # one 32-byte chain for all three: only the count and the modulus differ
    a, b, w = (mm.constants(curves.CURVES[n]) for n in ("bn254", "bls12_381", "bw6_761"))
    assert a[0] == int.from_bytes(mm.keccak256(mm.keccak256(b"seed")), "big") % curves.BN254.r
    assert w[:110] != a and all(x % curves.BN254.r == y for x, y in zip(w, a))  # 256-bit values are below BW6-761's r: unreduced


def test_empty_message_and_state():
    assert mm.mimc(curves.BN254, []) == 0 and mm.mimc(curves.BN254, [], 7) == 7
    e = [3, 5, 8]
    assert mm.mimc(curves.BN254, e) == mm.mimc(curves.BN254, e[2:], mm.mimc(curves.BN254, e[:2]))


@pytest.mark.parametrize("n", range(1, 41))
def test_levels_equal_the_subtree_stack(n):
    leaves = [b"leaf %d" % i for i in range(n)]
    lv = mm.levels(sha_H, leaves)
    assert [len(x) for x in lv][-1] == 1 and len(lv) - 1 == (n - 1).bit_length()
    for index in range(n):
        ref = mm.stack_tree(sha_H, leaves, index)
        got = mm.level_proof(lv, leaves, index)
        assert got == ref
        root, proof, idx, num = ref
        assert mm.verify_proof(sha_H, root, proof, idx, num)
        for k in range(1, len(proof)):  # a flipped sibling
            bad = list(proof)
            bad[k] = bytes([bad[k][0] ^ 1]) + bad[k][1:]
            assert not mm.verify_proof(sha_H, root, bad, idx, num)
        assert not mm.verify_proof(sha_H, root, [b"other"] + proof[1:], idx, num)
        assert not mm.verify_proof(sha_H, root, proof[:-1], idx, num) or len(proof) == 1
        assert not mm.verify_proof(sha_H, root, proof, num, num)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8])
def test_tree_over_mimc(n):
    c = curves.BN254
    H = mm.mimc_H(c)
    leaves = [(1000 + i).to_bytes(32, "big") + (i * i).to_bytes(32, "big") for i in range(n)]
    lv = mm.levels(H, leaves)
    for index in range(n):
        ref = mm.stack_tree(H, leaves, index)
        assert mm.level_proof(lv, leaves, index) == ref
        assert mm.verify_proof(H, *ref)
    # a leaf's sum is the MiMC of its elements, a node's of its two children
    assert lv[0][0] == mm.mimc(c, [1000, 0]).to_bytes(32, "big")
    if n >= 2:
        assert lv[1][0] == mm.mimc(c, [int.from_bytes(lv[0][0], "big"), int.from_bytes(lv[0][1], "big")]).to_bytes(32, "big")
    h = mm.Hash(c)
    h.Write(leaves[0])
    assert h.Sum() == lv[0][0]
