"""fr/fri's prover on the device against the big-int model (tests/fri_model.py) over the MiMC model: the whole ProofOfProximity and
OpeningProof byte for byte, at the smallest shapes at which each part can go wrong:
  - size 2: N = 16, one step, a 4-lane fold, a 16-leaf tree; size 3: padding to the next power of two;
  - size 64: N = 512 = MERKLE_TOP, tree 0 is k_merkle_top alone; size 128: N = 1024, the first k_merkle_level and the first sort
    to span more than one workgroup - the fold still runs in one (N / 4 = 256 = FRI_TPB lanes); BN254 also at 256;
  - size 256 (N = 2048, N / 4 = 512) on the two wider fields: the first fold over two workgroups there, checked as size 4096 is;
  - the reference test's size 4096 (BN254), where the pure-Python MiMC model is too slow: every layer against the model's field
    arithmetic, every root against a merkletree.DeviceTree over that layer, the proof through the host verifier, an opening
    against Horner;
  - edge inputs at sizes 2 and 64, the refusals that need a live domain or oracle, and the oracle's life cycle."""
import ctypes

import numpy as np
import pytest

import fri_model as fm
import mimc_model as mm
from conftest import random_scalars, rng_for
from test_gpu_gkr import dev, from_ints, to_ints

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
ARG = 4
CASES = [(c, s) for c in CURVES for s in (2, 3, 64, 128)] + [("bn254", 256)]
_models = {}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _poly(c, size, tag=0):
    return random_scalars(rng_for(0xF27, c.fr_limbs, size, tag), c, size)


def model(gm, curve, size, tag=0):
    """(params, hash, the polynomial's limbs, its integers, layers, trees, challenges, Evaluation, proof) computed once per case"""
    key = (curve, size, tag)
    if key not in _models:
        c = gm.CURVES[curve]
        P, h, p = fm.Params(c, size), fm.MiMC(c), _poly(c, size, tag)
        ints = to_ints(c, p)
        pre = fm.layers(P, h, ints)
        lay, trees, xs, evaluation, _, _ = pre
        _models[key] = (P, h, p, ints, lay, trees, xs, evaluation, fm.prove(P, h, ints, pre))
    return _models[key]


def same_proof(got, want):
    assert len(got.Rounds) == len(want.Rounds) == 1
    g, w = got.Rounds[0], want.Rounds[0]
    assert g.Evaluation == w.Evaluation and len(g.Interactions) == len(w.Interactions)
    for gi, wi in zip(g.Interactions, w.Interactions):
        for b in (0, 1):
            assert (gi[b].MerkleRoot, gi[b].ProofSet, gi[b].numLeaves) == (wi[b].MerkleRoot, wi[b].ProofSet, wi[b].numLeaves)


def same_opening(got, want):
    assert (got.merkleRoot, got.ProofSet, got.numLeaves, got.index, got.ClaimedValue) == \
        (want.merkleRoot, want.ProofSet, want.numLeaves, want.index, want.ClaimedValue)


def positions_of(P, tag):
    rng = rng_for(0xF28, P.N, tag)
    return sorted({0, P.N // 2 - 1, P.N // 2, P.N - 1} | {int(v) for v in rng.integers(0, P.N, 3)})


@pytest.mark.parametrize("curve,size", CASES)
def test_proof_and_openings_are_the_models(gm, curve, size):
    P, h, p, ints, _, trees, _, _, want = model(gm, curve, size)
    s = gm.fri.RADIX_2_FRI.New(curve, size, gm.mimc.Factory(curve))
    try:
        assert (s.nbSteps, s.Cardinality) == (P.nb_steps, P.N)
        got = s.BuildProofOfProximity(p)
        same_proof(got, want)
        s.VerifyProofOfProximity(got)
        fm.verify(P, h, got)
        for pos in positions_of(P, size):
            o = s.Open(p, pos)
            same_opening(o, fm.open_(P, h, ints, pos, trees[0]))
            s.VerifyOpening(pos, o, got)
            assert o.ClaimedValue == fm.horner(P, ints, pow(P.gen, pos, P.r))
    finally:
        s.Release()


def test_reference_size_4096(gm):
    """fri_test.go proves and opens at size 4096: N = 32768, 12 steps. No model hash: the layers are field arithmetic, the roots
    are held against the tree entry that is pinned on its own, the proof goes through the host verifier."""
    c, size = gm.BN254, 4096
    P = fm.Params(c, size)
    p = _poly(c, size)
    ints = to_ints(c, p)
    s = gm.fri.RADIX_2_FRI.New("bn254", size, gm.mimc.Factory("bn254"))
    o = s.Commit(p)
    try:
        xis, fs = s._transcript()
        fs.Bind(xis[0], bytes(32))
        cur, g_inv = fm.sort(fm.evaluations(P, ints)), P.gen_inv
        for i in range(P.nb_steps):
            layer = o.layer(i)
            assert layer.shape == (P.N >> i, 4) and to_ints(c, layer) == cur
            tree = gm.merkletree.DeviceTree(c, leaves=layer.reshape(-1, 1, 4), keep_leaves=False)
            try:
                assert tree.Root() == o.Root(i)
            finally:
                tree.Release()
            fs.Bind(xis[i], o.Root(i))
            xi = int.from_bytes(fs.ComputeChallenge(xis[i]), "big") % c.r
            out = o.fold(from_ints(c, [xi]))
            cur = fm.sort(fm.fold(cur, g_inv, xi, P))
            g_inv = g_inv * g_inv % c.r
            assert o.folds_done() == i + 1
        assert len(cur) == 8 and to_ints(c, out)[0] == cur[0]
        proof = s.BuildProofOfProximity(p)
        assert proof.Rounds[0].Evaluation == cur[0] and len(proof.Rounds[0].Interactions) == 12
        s.VerifyProofOfProximity(proof)
        m = int(rng_for(0xF29).integers(0, 1 << 62)) % 4096
        for opening in (s.Open(p, m), s.Open(o, m)):  # a second transform and tree, and one gather from the folded oracle
            s.VerifyOpening(m, opening, proof)
            assert opening.ClaimedValue == fm.horner(P, ints, pow(P.gen, m, c.r))
        same_opening(s.Open(p, m), s.Open(o, m))
    finally:
        o.Release()
        s.Release()


@pytest.mark.parametrize("curve", ["bls12_381", "bw6_761"])
def test_fold_across_workgroups(gm, curve):
    """size 256: N = 2048, so the first fold has N / 4 = 512 lanes, two workgroups of FRI_TPB = 256 (size 128 folds in one); only
    BN254 folds across workgroups elsewhere. As test_reference_size_4096, without the Python MiMC model: every layer against the
    model's field arithmetic, every root against a DeviceTree over that layer, the proof through the host verifier."""
    c, size = gm.CURVES[curve], 256
    P = fm.Params(c, size)
    assert P.N == 2048 and P.N // 4 == 2 * 256
    p = _poly(c, size)
    ints = to_ints(c, p)
    s = gm.fri.RADIX_2_FRI.New(curve, size, gm.mimc.Factory(curve))
    o = s.Commit(p)
    try:
        xis, fs = s._transcript()
        fs.Bind(xis[0], s._marshal(0))
        cur, g_inv = fm.sort(fm.evaluations(P, ints)), P.gen_inv
        for i in range(P.nb_steps):
            layer = o.layer(i)
            assert layer.shape == (P.N >> i, c.fr_limbs) and to_ints(c, layer) == cur, (curve, i)
            tree = gm.merkletree.DeviceTree(c, leaves=layer.reshape(-1, 1, c.fr_limbs), keep_leaves=False)
            try:
                assert tree.Root() == o.Root(i), (curve, i)
            finally:
                tree.Release()
            fs.Bind(xis[i], o.Root(i))
            xi = int.from_bytes(fs.ComputeChallenge(xis[i]), "big") % c.r
            out = o.fold(from_ints(c, [xi]))
            cur = fm.sort(fm.fold(cur, g_inv, xi, P))
            g_inv = g_inv * g_inv % c.r
            assert o.folds_done() == i + 1
        assert len(cur) == 8 and to_ints(c, out)[0] == cur[0]
        proof = s.BuildProofOfProximity(p)
        assert proof.Rounds[0].Evaluation == cur[0] and len(proof.Rounds[0].Interactions) == P.nb_steps == 8
        s.VerifyProofOfProximity(proof)
    finally:
        o.Release()
        s.Release()


# ------------------------------------------------------------------ edge inputs
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("size", [2, 64])
def test_inputs_from_the_device_short_and_zero(gm, curve, size):
    import torch
    c = gm.CURVES[curve]
    P, h, p, ints, _, trees, _, _, want = model(gm, curve, size)
    s = gm.fri.RADIX_2_FRI.New(curve, size, gm.mimc.Factory(curve))
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_p = dev(p)
            same_proof(s.BuildProofOfProximity(d_p=d_p.data_ptr(), n=size, stream=st.cuda_stream), want)
            same_opening(s.Open(None, P.N - 1, d_p=d_p.data_ptr(), n=size, stream=st.cuda_stream), fm.open_(P, h, ints, P.N - 1, trees[0]))
        assert (d_p.cpu().numpy().view(np.uint64).reshape(p.shape) == p).all()  # p is never modified
        # len(p) < size: the missing coefficients are zero; more than N coefficients: cut to N, as Go's copy does
        short = p[:size - 1]
        same_proof(s.BuildProofOfProximity(short), fm.prove(P, h, ints[:size - 1]))
        long = np.concatenate([p, np.zeros((P.N - size, c.fr_limbs), dtype=np.uint64), _poly(c, 3, 9)])
        same_proof(s.BuildProofOfProximity(long), want)
        # p all zero: every layer is zero
        zero = np.zeros((size, c.fr_limbs), dtype=np.uint64)
        got = s.BuildProofOfProximity(zero)
        same_proof(got, fm.prove(P, h, [0] * size))
        assert got.Rounds[0].Evaluation == 0
        s.VerifyProofOfProximity(got)
    finally:
        s.Release()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("size", [2, 64])
def test_fold_with_zero_and_minus_one(gm, curve, size):
    """xi = 0 and xi = r - 1 through gmsm_fri_fold itself, layer by layer against the model's fold"""
    c = gm.CURVES[curve]
    P, _, p, ints, _, _, _, _, _ = model(gm, curve, size)
    s = gm.fri.RADIX_2_FRI.New(curve, size, gm.mimc.Factory(curve))
    try:
        for first in (0, c.r - 1):
            xs = [(first, c.r - 1 - first, 12345)[k % 3] for k in range(P.nb_steps)]
            lay, _, _, evaluation, _, _ = fm.layers(P, None, ints, challenges=xs)
            o = s.Commit(p)
            try:
                for k in range(P.nb_steps):
                    assert to_ints(c, o.layer(k)) == lay[k]
                    out = o.fold(from_ints(c, [xs[k]]))
                assert to_ints(c, out)[0] == evaluation
            finally:
                o.Release()
    finally:
        s.Release()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("size", [2, 64])
def test_query_at_the_edges_and_open_from_an_oracle(gm, curve, size):
    c = gm.CURVES[curve]
    P, h, p, ints, lay, trees, xs, _, want = model(gm, curve, size)
    s = gm.fri.RADIX_2_FRI.New(curve, size, gm.mimc.Factory(curve))
    be = lambda v: v.to_bytes(P.bs, "big")
    o = s.Commit(p)
    try:
        same_proof(s.BuildProofOfProximity(o), want)  # folds the oracle with the challenges the model derived
        sizes = [P.N >> i for i in range(P.nb_steps)]
        rng = rng_for(0xF2A, size)
        for positions in ([2 * int(rng.integers(0, n // 2)) for n in sizes], [2 * int(rng.integers(0, n // 2)) + 1 for n in sizes],
                          [0] * P.nb_steps, [n - 1 for n in sizes]):
            pairs, sums, sibs, counts = o.query_limbs(positions)
            for i, pos in enumerate(positions):
                _, proof, _, _ = mm.level_proof(trees[i], [be(v) for v in lay[i]], pos)
                assert to_ints(c, pairs[i]) == lay[i][pos & ~1:(pos & ~1) + 2]
                assert be(to_ints(c, sums[i])[0]) == trees[i][0][pos]
                assert counts[i] == len(proof) - 1 == (P.N >> i).bit_length() - 1
                assert [be(v) for v in to_ints(c, sibs[i, :counts[i]])] == proof[1:] and not sibs[i, counts[i]:].any()
        # a prefix of the steps is a query too
        pairs, _, _, counts = o.query_limbs([1])
        assert to_ints(c, pairs[0]) == lay[0][:2] and counts[0] == P.N.bit_length() - 1
        for pos in positions_of(P, size + 1):
            same_opening(s.Open(o, pos), s.Open(p, pos))
            same_opening(s.Open(o, pos), fm.open_(P, h, ints, pos, trees[0]))
        with pytest.raises(ValueError, match="folded already"):
            s.BuildProofOfProximity(o)
    finally:
        o.Release()
        s.Release()


def test_layer_to_the_device(gm):
    import torch
    c = gm.BN254
    P, _, p, _, lay, _, xs, _, _ = model(gm, "bn254", 64)
    s = gm.fri.RADIX_2_FRI.New("bn254", 64, gm.mimc.Factory("bn254"))
    o = s.Commit(p)
    try:
        o.fold(from_ints(c, [xs[0]]))
        for step in (0, 1):
            n = P.N >> step
            d = torch.full(((n + 1) * c.fr_limbs,), 9, dtype=torch.int64, device="cuda")
            o.layer_device(step, d.data_ptr())
            got = d.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs)
            assert to_ints(c, got[:n]) == lay[step] and (got[n] == 9).all()  # the element behind the layer is not written
    finally:
        o.Release()
        s.Release()


# ------------------------------------------------------------------ refusals and the life cycle
def test_refusals_write_nothing(gm):
    c = gm.BN254
    lib = gm._lib.load()
    err = gm._lib.last_error
    a = np.full((40, 4), 7, dtype=np.uint64)
    out = np.full((40, 4), 9, dtype=np.uint64)
    cnt = np.full(4, 9, dtype=np.uint32)
    handle = ctypes.c_uint64(77)
    small, dom = gm.fft.NewDomain(c, 8), gm.fft.NewDomain(c, 32)
    E = "gmsm_fri_commit: "
    commit = lib.gmsm_fri_commit
    assert commit(small.handle, _p(a), None, 8, None, ctypes.byref(handle)) == ARG
    assert err() == E + "the domain's cardinality 8 is below 16 (rho = 8 times a size of at least 2)"
    assert commit(dom.handle, _p(a), None, 33, None, ctypes.byref(handle)) == ARG and err() == E + "len = 33 is more than the domain's cardinality 32"
    assert commit(dom.handle, _p(a), None, 4, None, None) == ARG and err() == E + "out_oracle is null"
    assert commit(dom.handle, None, None, 4, None, ctypes.byref(handle)) == ARG and err() == E + "give exactly one of p (host) / d_p (device)"
    assert commit(dom.handle, _p(a), 4096, 4, None, ctypes.byref(handle)) == ARG and err() == E + "give exactly one of p (host) / d_p (device)"
    assert handle.value == 77
    p = _poly(c, 4)
    assert commit(dom.handle, _p(p), None, 4, None, ctypes.byref(handle)) == 0  # N = 32: two steps
    h = handle.value
    card, steps, done = ctypes.c_uint64(0), ctypes.c_uint(0), ctypes.c_uint(9)
    assert lib.gmsm_fri_info(h, ctypes.byref(card), ctypes.byref(steps), ctypes.byref(done)) == 0
    assert (card.value, steps.value, done.value) == (32, 2, 0)
    pos = np.array([0, 0], dtype=np.uint64)
    query = lambda count: lib.gmsm_fri_query(h, _p(pos), count, _p(out), _p(out[4:]), _p(out[8:]), _p(cnt))
    # before the first fold one layer is built: its root, layer and query are there, step 1 is not
    assert lib.gmsm_fri_root(h, 1, _p(out)) == ARG and err() == "gmsm_fri_root: step 1 is not built (1 of 2 layers are)"
    assert lib.gmsm_fri_layer(h, 1, _p(out), None) == ARG and err() == "gmsm_fri_layer: step 1 is not built (1 of 2 layers are)"
    assert query(2) == ARG and err() == "gmsm_fri_query: step 1 is not built (1 of 2 layers are)"
    assert lib.gmsm_fri_root(h, 0, None) == ARG and err() == "gmsm_fri_root: out_root is null"
    assert lib.gmsm_fri_layer(h, 0, None, None) == ARG and err() == "gmsm_fri_layer: give exactly one of out (host) / d_out (device)"
    assert lib.gmsm_fri_layer(h, 0, _p(out), 4096) == ARG and err() == "gmsm_fri_layer: give exactly one of out (host) / d_out (device)"
    assert lib.gmsm_fri_fold(h, None, _p(out)) == ARG and err() == "gmsm_fri_fold: xi and out must not be null"
    assert lib.gmsm_fri_fold(h, _p(a), None) == ARG and err() == "gmsm_fri_fold: xi and out must not be null"
    assert lib.gmsm_fri_query(h, _p(pos), 1, _p(out), None, _p(out), _p(cnt)) == ARG and err() == "gmsm_fri_query: positions and the four outputs must not be null"
    pos[0] = 32
    assert query(1) == ARG and err() == "gmsm_fri_query: positions[0] = 32 is outside [0, 32)"
    assert (out == 9).all() and (cnt == 9).all()
    pos[0] = 31
    assert query(0) == 0 and (out == 9).all()
    assert query(1) == 0 and cnt[0] == 5
    xi = from_ints(c, [3])
    root1 = np.zeros(4, dtype=np.uint64)
    assert lib.gmsm_fri_fold(h, _p(xi), _p(root1)) == 0
    pos[1] = 16
    out[:] = 9
    cnt[:] = 9
    assert query(2) == ARG and err() == "gmsm_fri_query: positions[1] = 16 is outside [0, 16)" and (out == 9).all() and (cnt == 9).all()
    pos[1] = 15
    assert query(2) == 0 and list(cnt[:2]) == [5, 4]
    got = np.zeros(4, dtype=np.uint64)
    assert lib.gmsm_fri_root(h, 1, _p(got)) == 0 and (got == root1).all()
    assert lib.gmsm_fri_fold(h, _p(xi), _p(got)) == 0  # the last fold: the Evaluation, no tree
    assert lib.gmsm_fri_info(h, None, None, ctypes.byref(done)) == 0 and done.value == 2
    assert lib.gmsm_fri_root(h, 2, _p(got)) == ARG and err() == "gmsm_fri_root: step 2 is not built (2 of 2 layers are)"
    keep = got.copy()
    assert lib.gmsm_fri_fold(h, _p(xi), _p(got)) == ARG and err() == "gmsm_fri_fold: all 2 folds are done" and (got == keep).all()
    assert lib.gmsm_fri_release(h) == 0
    for call in (lambda: lib.gmsm_fri_root(h, 0, _p(got)), lambda: lib.gmsm_fri_fold(h, _p(xi), _p(got)), lambda: lib.gmsm_fri_layer(h, 0, _p(out), None),
                 lambda: query(1), lambda: lib.gmsm_fri_info(h, None, None, None), lambda: lib.gmsm_fri_release(h)):
        assert call() == ARG and err() == "unknown fri oracle handle"
    small.release()
    dom.release()


def test_two_oracles_over_one_domain_and_a_released_domain(gm):
    c = gm.BN254
    P, _, p, ints, lay, _, xs, evaluation, want = model(gm, "bn254", 64)
    _, _, p2, ints2, lay2, _, xs2, evaluation2, want2 = model(gm, "bn254", 64, tag=1)
    s = gm.fri.RADIX_2_FRI.New("bn254", 64, gm.mimc.Factory("bn254"))
    a, b = s.Commit(p), s.Commit(p2)
    s.Release()  # the oracles keep the domain alive
    gm.trim(0)   # and their memory is in use
    try:
        for k in range(P.nb_steps):  # fold them in turn
            assert to_ints(c, a.layer(k)) == lay[k] and to_ints(c, b.layer(k)) == lay2[k]
            oa, ob = a.fold(from_ints(c, [xs[k]])), b.fold(from_ints(c, [xs2[k]]))
        assert to_ints(c, oa)[0] == evaluation and to_ints(c, ob)[0] == evaluation2
        assert [a.Root(k) for k in range(P.nb_steps)] == [r[0].MerkleRoot for r in want.Rounds[0].Interactions]
        assert [b.Root(k) for k in range(P.nb_steps)] == [r[0].MerkleRoot for r in want2.Rounds[0].Interactions]
    finally:
        a.Release()
        b.Release()
    with pytest.raises(ValueError, match="unknown fri oracle handle"):
        a.Root(0)


def test_shutdown_with_a_live_oracle(gm):
    c = gm.BN254
    _, _, p, _, _, _, _, _, want = model(gm, "bn254", 2)
    s = gm.fri.RADIX_2_FRI.New("bn254", 2, gm.mimc.Factory("bn254"))
    o = s.Commit(p)
    assert o.Root(0) == want.Rounds[0].Interactions[0][0].MerkleRoot
    gm.shutdown()
    for call in (lambda: o.Root(0), lambda: o.fold(from_ints(c, [1])), lambda: o.layer(0), o.Release):
        with pytest.raises(ValueError, match="unknown fri oracle handle"):
            call()
    s._domain = None  # drained with everything else
    again = gm.fri.RADIX_2_FRI.New("bn254", 2, gm.mimc.Factory("bn254"))  # the library is usable again
    same_proof(again.BuildProofOfProximity(p), want)
    again.Release()
