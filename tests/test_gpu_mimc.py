"""MiMC batches and Merkle trees on the device against the big-int model (tests/mimc_model.py), exact equality of canonical limbs
and bytes, at the smallest shapes at which each kernel can go wrong:
  - k_mimc_batch: one message, one short of / exactly / one over a wave, more than one workgroup (257); no block, one, two, five;
    messages packed and 3 elements apart; host and device pointers on a non-default stream; from 0 and from a state; the row
    behind the output is not written; the reference's ten BN254 vectors as one batch per length;
  - the tree: n = 1 (no level), 2, odd and even small n, 255 / 256 / 257, either side of the size k_merkle_top takes alone (512,
    513: one k_merkle_level launch first) and 4097 (four launches, an orphan that moves up through every one of them); leaves
    of one and of three elements; built from the host with the leaves kept and from the device without;
  - gkr.Prove over a Fiat-Shamir transcript that hashes with mimc.NewMiMC: the model's proof, which the model's verifier accepts."""
import ctypes
import json
import os

import numpy as np
import pytest

import gkr_model as M
import mimc_model as mm
from conftest import random_scalars, rng_for
from test_gpu_gkr import back, dev, from_ints, mimc as mimc_gate, prove_on_device, to_ints

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
HERE = os.path.dirname(os.path.abspath(__file__))
ARG = 4
COUNTS = [1, 63, 64, 65, 257]
TOP = 512  # MERKLE_TOP (gmsm_mimc.h): the largest level k_merkle_top takes


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("length", [0, 1, 2, 5])
@pytest.mark.parametrize("pad", [0, 3])
def test_sum_batch(gm, curve, length, pad):
    import torch
    c = gm.CURVES[curve]
    lib = gm._lib.load()
    gid = gm._lib.GROUP_IDS[(curve, "g1")]
    rng = rng_for(0x313C, CURVES.index(curve), length, pad)
    stride, most = length + pad, max(COUNTS)
    data = random_scalars(rng, c, max(most * stride, 1))
    state = random_scalars(rng, c, 1)
    ints, st = to_ints(c, data), to_ints(c, state)[0]
    expected = {h0: from_ints(c, [mm.mimc(c, ints[i * stride:i * stride + length], h0) for i in range(most)]) for h0 in (0, st)}
    d_data = dev(data)
    s = torch.cuda.Stream()
    for count in COUNTS:
        for h0, state_arg in ((0, None), (st, state)):
            sp = None if state_arg is None else _p(state_arg)
            out = np.full((count + 1, c.fr_limbs), 9, dtype=np.uint64)
            assert lib.gmsm_mimc_sum_batch(gid, _p(data) if length else None, None, count, length, stride, sp, None, _p(out), None) == 0, gm._lib.last_error()
            assert (out[:count] == expected[h0][:count]).all() and (out[count] == 9).all()
            with torch.cuda.stream(s):
                d_out = dev(np.full((count + 1, c.fr_limbs), 9, dtype=np.uint64))
                d_in = d_data * 1  # produced on this stream
                gm.mimc.sum_batch_device(c, d_in.data_ptr(), count, length, stride, d_out.data_ptr(), state=state_arg, stream=s.cuda_stream)
            got = back(d_out, c)  # the call has returned: its result is complete
            assert (got[:count] == expected[h0][:count]).all() and (got[count] == 9).all()
            assert (back(d_in, c) == data).all()
    if length and not pad:
        msgs = data[:65 * length].reshape(65, length, c.fr_limbs)
        assert (gm.mimc.SumBatch(c, msgs) == expected[0][:65]).all()
        assert (gm.mimc.SumBatch(c, msgs, state=state) == expected[st][:65]).all()


def test_the_reference_vectors_as_batches(gm):
    with open(os.path.join(HERE, "golden", "mimc_vectors.json")) as f:
        vs = json.load(f)["bn254"]
    c = gm.BN254
    by_len = {}
    for v in vs:
        by_len.setdefault(len(v["in"]), []).append(v)
    assert sorted(by_len) == [1, 2, 3, 4, 5] and sum(len(g) for g in by_len.values()) == 10
    for length, group in by_len.items():
        msgs = np.stack([from_ints(c, [int(x, 16) for x in v["in"]]) for v in group])
        assert to_ints(c, gm.mimc.SumBatch(c, msgs)) == [int(v["out"], 16) for v in group]


def test_sum_batch_refuses_overlapping_device_vectors(gm):
    c = gm.BN254
    d = dev(np.zeros((16, c.fr_limbs), dtype=np.uint64))
    with pytest.raises(ValueError) as e:
        gm.mimc.sum_batch_device(c, d.data_ptr(), 4, 2, 2, d.data_ptr() + 4 * 32)
    assert str(e.value) == "gmsm_mimc_sum_batch: the output overlaps an input (inputs are never modified)"
    gm.mimc.sum_batch_device(c, d.data_ptr(), 4, 2, 2, d.data_ptr() + 8 * 32)  # right behind the input: fine
    assert to_ints(c, back(d, c)[8:12]) == [mm.mimc(c, [0, 0])] * 4


# ------------------------------------------------------------------ trees
def leaf_ints(c, i, leaf_len):
    return [pow(i * 7919 + j * 104729 + 12345, 3, c.r) for j in range(leaf_len)]


_leaf_sums = {}


def model_levels(c, n, leaf_len):
    """the model's levels as integers; the leaves' sums are shared by every n (leaf i does not depend on n)"""
    sums = _leaf_sums.setdefault((c.name, leaf_len), [])
    while len(sums) < n:
        sums.append(mm.mimc(c, leaf_ints(c, len(sums), leaf_len)))
    lv = [sums[:n]]
    while len(lv[-1]) > 1:
        cur = lv[-1]
        lv.append([mm.mimc(c, cur[i:i + 2]) if i + 1 < len(cur) else cur[i] for i in range(0, len(cur), 2)])
    return lv


def proof_indices(n):
    idx = {0, n - 1, (1 << (n.bit_length() - 1)) - 1}  # first, last (an orphan when n is odd), the last of the largest complete subtree
    if n >= 2:
        idx.add(n - 2)  # for n = 7, 4097 ..: its parent's sibling is the orphan, moved up
    if n > 4:
        idx.add(n - 1 - (n - 1) % 4)  # the first leaf of the last group of four: an orphan higher up when that group is short
    return sorted(idx)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 255, 256, 257, TOP, TOP + 1, 4097])
@pytest.mark.parametrize("leaf_len", [1, 3])
def test_tree(gm, curve, n, leaf_len):
    import torch
    c = gm.CURVES[curve]
    bs = 8 * c.fr_limbs
    be = lambda v: v.to_bytes(bs, "big")
    lv = model_levels(c, n, leaf_len)
    assert len(lv) - 1 == (n - 1).bit_length()
    blv = [[be(v) for v in level] for level in lv]
    leaves_b = [b"".join(be(v) for v in leaf_ints(c, i, leaf_len)) for i in range(n)]
    leaves = from_ints(c, [v for i in range(n) for v in leaf_ints(c, i, leaf_len)]).reshape(n, leaf_len, c.fr_limbs)
    indices = proof_indices(n)
    expected = [mm.level_proof(blv, leaves_b, i) for i in indices]
    h = gm.mimc.NewMiMC(curve)

    kept = gm.merkletree.DeviceTree(c, leaves=leaves, leaf_len=leaf_len, keep_leaves=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_leaves = dev(leaves)
        bare = gm.merkletree.DeviceTree(c, d_leaves=d_leaves.data_ptr(), n=n, leaf_len=leaf_len, keep_leaves=False, stream=s.cuda_stream)
    try:
        for t in (kept, bare):
            assert (t.n, t.leaf_len, t.depth) == (n, leaf_len, len(lv) - 1)
            assert t.Root() == blv[-1][0]
        assert kept.Prove(indices) == expected
        assert bare.Prove(indices, leaf_data=leaves[indices]) == expected
        for root, proof, index, num in expected:
            assert gm.merkletree.VerifyProof(h, root, proof, index, num)
            assert len(proof) - 1 <= kept.depth
        root, proof, index, num = expected[-1]
        if len(proof) > 1:
            assert not gm.merkletree.VerifyProof(h, root, proof[:1] + [proof[1][:-1] + bytes([proof[1][-1] ^ 1])] + proof[2:], index, num)  # the lowest bit: still canonical
        # the slots behind a short path are zero, the counts are the paths' lengths
        _, sibs, counts = kept.prove_limbs(indices)
        for j, (_, proof, _, _) in enumerate(expected):
            assert counts[j] == len(proof) - 1 and not sibs[j, counts[j]:].any()
        assert (back(d_leaves, c).reshape(leaves.shape) == leaves).all()
        # without the leaves: refused before any device work, nothing written
        with pytest.raises(ValueError):
            bare.Prove(indices)
        lib = gm._lib.load()
        idx = np.array(indices, dtype=np.uint64)
        out_l = np.full((len(idx), leaf_len, c.fr_limbs), 9, dtype=np.uint64)
        out_s = np.full((len(idx), max(bare.depth, 1), c.fr_limbs), 9, dtype=np.uint64)
        cnt = np.full(len(idx), 9, dtype=np.uint32)
        assert lib.gmsm_merkle_prove(bare.handle, _p(idx), len(idx), _p(out_l), _p(out_s), _p(cnt)) == ARG
        assert gm._lib.last_error() == "gmsm_merkle_prove: out_leaves is given, but the tree was built without keep_leaves"
        idx[-1] = n
        assert lib.gmsm_merkle_prove(kept.handle, _p(idx), len(idx), _p(out_l), _p(out_s), _p(cnt)) == ARG
        assert gm._lib.last_error() == "gmsm_merkle_prove: indices[%d] = %d is outside [0, %d)" % (len(idx) - 1, n, n)
        assert (out_l == 9).all() and (out_s == 9).all() and (cnt == 9).all()
        assert lib.gmsm_merkle_prove(kept.handle, _p(idx), 0, None, None, None) == 0
    finally:
        kept.Release()
        bare.Release()
    for t in (kept, bare):  # release, then use
        for call in (t.Root, lambda: t.Prove(indices[:1], leaf_data=leaves[indices[:1]]), t.Release):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "unknown merkle tree handle"


def test_trees_survive_trim_and_run_side_by_side(gm):
    c = gm.BN254
    n = 37
    lv = model_levels(c, n, 1)
    leaves = from_ints(c, [leaf_ints(c, i, 1)[0] for i in range(n)]).reshape(n, 1, c.fr_limbs)
    a = gm.merkletree.DeviceTree(c, leaves=leaves)
    b = gm.merkletree.DeviceTree(c, leaves=leaves[:8])
    try:
        gm.trim(0)
        assert a.Root() == lv[-1][0].to_bytes(32, "big") and b.Root() == model_levels(c, 8, 1)[-1][0].to_bytes(32, "big")
        h = gm.mimc.NewMiMC("bn254")
        for t in (a, b):
            for root, proof, index, num in t.Prove(range(t.n)):
                assert gm.merkletree.VerifyProof(h, root, proof, index, num)
    finally:
        a.Release()
        b.Release()


def test_shutdown_releases_trees(gm):
    c = gm.BN254
    leaves = from_ints(c, [leaf_ints(c, i, 1)[0] for i in range(8)]).reshape(8, 1, c.fr_limbs)
    root = model_levels(c, 8, 1)[-1][0].to_bytes(32, "big")
    t = gm.merkletree.DeviceTree(c, leaves=leaves)
    assert t.Root() == root
    gm.shutdown()
    for call in (t.Root, lambda: t.Prove([0]), t.Release):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "unknown merkle tree handle"
    again = gm.merkletree.DeviceTree(c, leaves=leaves)  # the library is usable again
    assert again.Root() == root and again.handle != t.handle
    again.Release()


# ------------------------------------------------------------------ GKR over a MiMC transcript
class ModelMiMC:
    """the model's digest with hashlib's method names, as gkr_model's transcript calls it"""

    def __init__(self, c):
        self.c, self.bs, self.data = c, 8 * c.fr_limbs, []

    def update(self, p):
        if 0 < len(p) < self.bs:
            p = bytes(self.bs - len(p)) + p
        assert len(p) % self.bs == 0
        self.data += [int.from_bytes(p[i:i + self.bs], "big") for i in range(0, len(p), self.bs)]

    def digest(self):
        return mm.mimc(self.c, self.data).to_bytes(self.bs, "big")


@pytest.mark.parametrize("curve", CURVES)
def test_gkr_over_a_mimc_transcript(gm, curve):
    """a two-level MiMC chain; input 0 feeds both levels, so it has two claims and a comb challenge"""
    c = gm.CURVES[curve]
    F = M.Field(c.r, c.fr_limbs * 8)
    rng = rng_for(0x313D, CURVES.index(curve))
    n = 1 << 4
    circuit = [(None, []), (None, []), ("mimc", [1, 0]), ("mimc", [2, 0])]
    inputs = {j: to_ints(c, random_scalars(rng, c, n)) for j in (0, 1)}
    full = M.complete(circuit, [inputs[0], inputs[1], None, None], F.p)
    model_hash = lambda: ModelMiMC(c)
    expected = M.prove(F, circuit, full, model_hash)
    assert any(name.endswith("comb") for name in M.challenge_names(M.Sorted(circuit), 4))
    proof, got_full = prove_on_device(gm, c, circuit, inputs, gm.mimc.Factory(curve), True)
    assert proof == expected and got_full == full
    assert M.verify(F, circuit, full, proof, model_hash) is None
    assert M.verify(F, circuit, full, proof, gm.mimc.Factory(curve)) is None
    assert mimc_gate(2, 3) == 5 ** 7  # the gate of the circuit is the hash's round without its constant
