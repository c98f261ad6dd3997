"""The MiMC and Merkle entries of include/gmsm.h without a device: the eight symbols are exported, declared with the stated
arity and bound; gmsm_mimc_constants and gmsm_mimc_hash (host arithmetic) equal the big-int model on all three curves; mimc.NewMiMC
keeps the reference's Write rules and error texts; every error the host can decide returns GMSM_ERR_ARG with its text
before any device work, and nothing is written."""
import ctypes
import re
import os

import numpy as np
import pytest

import mimc_model as mm
from conftest import rng_for, random_scalars, scalars_from_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITIES = {"gmsm_mimc_constants": 3, "gmsm_mimc_hash": 5, "gmsm_mimc_sum_batch": 10, "gmsm_merkle_new": 8, "gmsm_merkle_info": 4,
           "gmsm_merkle_root": 2, "gmsm_merkle_prove": 6, "gmsm_merkle_release": 1}
ARG = 4  # GMSM_ERR_ARG
CURVES = ["bn254", "bls12_381", "bw6_761"]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_are_exported_declared_and_bound(gm):
    lib = gm._lib.load()
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        decls = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for sym, arity in ARITIES.items():
        assert sym in gm._lib.ABI_SYMBOLS
        f = getattr(lib, sym)
        assert f.restype is ctypes.c_int
        proto = re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
        assert proto, sym
        assert len(f.argtypes) == proto.group(1).count(",") + 1 == arity, sym


@pytest.mark.parametrize("name", CURVES)
def test_constants_equal_the_model(gm, name):
    c = gm.CURVES[name]
    lib = gm._lib.load()
    for gid in (gm._lib.GROUP_IDS[(name, "g1")], gm._lib.GROUP_IDS[(name, "g2")]):  # a G2 id names the same scalar field
        rounds = ctypes.c_uint(0)
        assert lib.gmsm_mimc_constants(gid, None, ctypes.byref(rounds)) == 0 and rounds.value == mm.ROUNDS[name]
        out = np.zeros((rounds.value, c.fr_limbs), dtype=np.uint64)
        assert lib.gmsm_mimc_constants(gid, _p(out), None) == 0
        assert (out == scalars_from_ints(c, mm.constants(c))).all()
    assert gm.mimc.GetConstants(name) == mm.constants(c)


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("length", [0, 1, 5])
def test_hash_equals_the_model(gm, name, length):
    c = gm.CURVES[name]
    lib = gm._lib.load()
    gid = gm._lib.GROUP_IDS[(name, "g1")]
    rng = rng_for(0x3131, CURVES.index(name), length)
    elems = random_scalars(rng, c, max(length, 1))[:length]
    state = random_scalars(rng, c, 1)
    ints = [gm.polynomial.to_int(c, e) for e in elems]
    for st in (None, state):
        out = np.zeros(c.fr_limbs, dtype=np.uint64)
        assert lib.gmsm_mimc_hash(gid, None if st is None else _p(st), _p(elems) if length else None, length, _p(out)) == 0
        h0 = 0 if st is None else gm.polynomial.to_int(c, st)
        assert gm.polynomial.to_int(c, out) == mm.mimc(c, ints, h0)
        assert (out == scalars_from_ints(c, [mm.mimc(c, ints, h0)])[0]).all()  # canonical limbs


def test_new_mimc_reproduces_the_vectors_and_the_write_rules(gm):
    import json
    with open(os.path.join(ROOT, "tests", "golden", "mimc_vectors.json")) as f:
        vs = json.load(f)["bn254"]
    c = gm.BN254
    be = lambda v: v.to_bytes(32, "big")
    for v in vs:
        msg = b"".join(be(int(x, 16)) for x in v["in"])
        assert gm.mimc.Sum("bn254", msg) == be(int(v["out"], 16))
        h = gm.mimc.NewMiMC("bn254")
        for x in v["in"]:  # block by block
            h.update(be(int(x, 16)))
        assert h.digest() == be(int(v["out"], 16)) == h.digest()  # Sum flushes the data: a second one adds nothing
        le = gm.mimc.NewMiMC("bn254", byte_order="little")
        le.Write(b"".join(int(x, 16).to_bytes(32, "little") for x in v["in"]))
        assert le.Sum() == be(int(v["out"], 16))  # the output stays big-endian
    h = gm.mimc.NewMiMC("bn254")
    assert h.Sum() == bytes(32) and h.Size() == h.BlockSize() == 32  # an empty message gives 0
    # shorter than one block: left-padded with zeros
    h.Write(b"\x01\x02")
    assert h.Sum() == be(mm.mimc(c, [0x0102]))
    h.Reset()
    assert h.Write(b"") == 0 and h.Sum() == bytes(32)
    # the two errors
    with pytest.raises(ValueError) as e:
        h.Write(be(c.r))
    assert str(e.value) == "invalid fr.Element encoding"
    with pytest.raises(ValueError) as e:
        h.Write(bytes(33))
    assert str(e.value) == "invalid input length: must represent a list of field elements, expects a []byte of len m*BlockSize"
    assert h.Sum() == bytes(32)  # nothing was taken in
    h.Write(be(c.r - 1))
    assert h.Sum() == be(mm.mimc(c, [c.r - 1]))
    # State / SetState
    h = gm.mimc.NewMiMC("bn254")
    h.Write(be(3) + be(5))
    mid = h.State()
    assert mid == be(mm.mimc(c, [3, 5]))
    g = gm.mimc.NewMiMC("bn254")
    g.SetState(mid)
    g.Write(be(8))
    assert g.Sum() == be(mm.mimc(c, [3, 5, 8])) and g.State() == g.Sum()
    with pytest.raises(ValueError) as e:
        g.SetState(bytes(31))
    assert str(e.value) == "the mimc state expects a state of 32 bytes"
    with pytest.raises(ValueError) as e:
        g.SetState(be(c.r))
    assert str(e.value) == "the provided newState does not represent a valid state"
    w = gm.mimc.NewMiMC("bw6_761")
    assert w.BlockSize() == 48
    w.Write((7).to_bytes(48, "big"))
    assert w.Sum() == mm.mimc(gm.BW6_761, [7]).to_bytes(48, "big")


def test_new_mimc_fits_the_transcript(gm):
    c = gm.BLS12_381
    t = gm.fiatshamir.NewTranscript(gm.mimc.Factory("bls12_381"), "alpha", "beta")
    t.Bind("alpha", (11).to_bytes(32, "big"))
    t.Bind("beta", (12).to_bytes(32, "big"))
    a = t.ComputeChallenge("alpha")
    b = t.ComputeChallenge("beta")
    name = lambda s: int.from_bytes(s.encode(), "big")
    assert a == mm.mimc(c, [name("alpha"), 11]).to_bytes(32, "big")
    assert b == mm.mimc(c, [name("beta"), int.from_bytes(a, "big"), 12]).to_bytes(32, "big")


def test_verify_proof_on_the_host(gm):
    c = gm.BN254
    H = mm.mimc_H(c)
    leaves = [(50 + i).to_bytes(32, "big") for i in range(5)]
    lv = mm.levels(H, leaves)
    h = gm.mimc.NewMiMC("bn254")
    for index in range(5):
        root, proof, idx, num = mm.level_proof(lv, leaves, index)
        assert gm.merkletree.VerifyProof(h, root, proof, idx, num)
        if len(proof) > 1:
            bad = proof[:1] + [proof[1][:-1] + bytes([proof[1][-1] ^ 1])] + proof[2:]  # the lowest bit: still canonical
            assert not gm.merkletree.VerifyProof(h, root, bad, idx, num)
        assert not gm.merkletree.VerifyProof(h, root, proof, 5, num) and not gm.merkletree.VerifyProof(h, None, proof, idx, num)
        assert not gm.merkletree.VerifyProof(h, root, [], idx, num)


def test_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    a = np.full((8, 4), 7, dtype=np.uint64)
    out = np.full((8, 4), 9, dtype=np.uint64)
    rounds = ctypes.c_uint(5)
    assert lib.gmsm_mimc_constants(99, _p(out), ctypes.byref(rounds)) == ARG and "unknown group" in err()
    assert lib.gmsm_mimc_constants(0, None, None) == ARG and err() == "gmsm_mimc_constants: out and out_rounds are both null"
    E = "gmsm_mimc_hash: "
    assert lib.gmsm_mimc_hash(99, None, _p(a), 2, _p(out)) == ARG and "unknown group" in err()
    assert lib.gmsm_mimc_hash(0, None, _p(a), 2, None) == ARG and err() == E + "out is null"
    assert lib.gmsm_mimc_hash(0, None, None, 2, _p(out)) == ARG and err() == E + "elems is null"
    E = "gmsm_mimc_sum_batch: "
    sb = lib.gmsm_mimc_sum_batch
    assert sb(99, _p(a), None, 4, 2, 2, None, None, _p(out), None) == ARG and "unknown group" in err()
    assert sb(0, None, None, 0, 2, 1, None, None, None, None) == 0  # count == 0 touches nothing, whatever else is given
    assert sb(0, _p(a), None, 4, 2, 1, None, None, _p(out), None) == ARG and err() == E + "stride = 1 is less than len = 2"
    assert sb(0, None, None, 4, 2, 2, None, None, _p(out), None) == ARG and err() == E + "give exactly one of msgs (host) / d_msgs (device)"
    assert sb(0, _p(a), 4096, 4, 2, 2, None, None, _p(out), None) == ARG and err() == E + "give exactly one of msgs (host) / d_msgs (device)"
    assert sb(0, _p(a), 4096, 4, 0, 2, None, None, _p(out), None) == ARG and err() == E + "give at most one of msgs (host) / d_msgs (device)"
    assert sb(0, _p(a), None, 4, 2, 2, None, None, None, None) == ARG and err() == E + "give exactly one of out (host) / d_out (device)"
    assert sb(0, _p(a), None, 4, 2, 2, None, None, _p(out), 4096) == ARG and err() == E + "give exactly one of out (host) / d_out (device)"
    assert sb(0, _p(a), None, 1 << 61, 2, 2, None, None, _p(out), None) == ARG and err() == E + "count * stride does not fit"
    assert sb(0, _p(a), None, 4, 1, 1 << 60, None, None, _p(out), None) == ARG and err() == E + "count * stride does not fit"
    assert sb(0, _p(a), None, 4, 2, 2, None, None, _p(a[3:]), None) == ARG and err() == E + "the output overlaps an input (inputs are never modified)"
    assert sb(0, _p(a), None, 4, 2, 2, None, None, _p(a), None) == ARG
    assert (a == 7).all() and (out == 9).all()
    # len == 0 on the host: count copies of the state, with no device
    st = scalars_from_ints(gm.BN254, [12345])
    assert sb(0, None, None, 3, 0, 0, _p(st), None, _p(out), None) == 0 and (out[:3] == st[0]).all() and (out[3:] == 9).all()
    assert sb(0, None, None, 2, 0, 5, None, None, _p(out), None) == 0 and (out[:2] == 0).all() and (out[2] == st[0]).all()
    E = "gmsm_merkle_new: "
    handle = ctypes.c_uint64(77)
    mn = lib.gmsm_merkle_new
    assert mn(99, _p(a), None, 4, 2, 1, None, ctypes.byref(handle)) == ARG and "unknown group" in err()
    assert mn(0, _p(a), None, 0, 2, 1, None, ctypes.byref(handle)) == ARG and err() == E + "no leaf (n == 0)"
    assert mn(0, _p(a), None, 4, 0, 1, None, ctypes.byref(handle)) == ARG and err() == E + "empty leaves (leaf_len == 0)"
    assert mn(0, _p(a), None, 4, 2, 1, None, None) == ARG and err() == E + "out_handle is null"
    assert mn(0, None, None, 4, 2, 1, None, ctypes.byref(handle)) == ARG and err() == E + "give exactly one of leaves (host) / d_leaves (device)"
    assert mn(0, _p(a), 4096, 4, 2, 1, None, ctypes.byref(handle)) == ARG and err() == E + "give exactly one of leaves (host) / d_leaves (device)"
    assert mn(0, _p(a), None, 1 << 59, 1 << 10, 1, None, ctypes.byref(handle)) == ARG and err() == E + "n * leaf_len does not fit"
    assert handle.value == 77
    n, ll, depth = ctypes.c_size_t(1), ctypes.c_size_t(2), ctypes.c_uint(3)
    idx = np.zeros(2, dtype=np.uint64)
    cnt = np.full(2, 9, dtype=np.uint32)
    for h in (0, 1, 1 << 40):
        assert lib.gmsm_merkle_info(h, ctypes.byref(n), ctypes.byref(ll), ctypes.byref(depth)) == ARG and err() == "unknown merkle tree handle"
        assert lib.gmsm_merkle_root(h, _p(out)) == ARG and err() == "unknown merkle tree handle"
        assert lib.gmsm_merkle_prove(h, _p(idx), 2, None, _p(out), _p(cnt)) == ARG and err() == "unknown merkle tree handle"
        assert lib.gmsm_merkle_release(h) == ARG and err() == "unknown merkle tree handle"
    assert (n.value, ll.value, depth.value) == (1, 2, 3) and (out[3:] == 9).all() and (cnt == 9).all()
