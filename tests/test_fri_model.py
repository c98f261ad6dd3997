"""fr/fri without a device: the big-int model (fri_model.py) proves and verifies over sha256 (the reference's own test hash) and over
the MiMC model; its openings claim the polynomial's value; deriveQueriesPositions keeps the fibres; the two index identities the
kernels rest on equal the plain two-pass forms; and the package's host verifiers (fri.VerifyProofOfProximity, fri.VerifyOpening)
accept the model's proofs under both hashes and reject each tampering with the reference's error."""
import copy
import hashlib

import pytest

import fri_model as fm
import mimc_model as mm
from conftest import rng_for

SIZES = [2, 3, 4, 64, 100]
HASHES = ["sha256", "mimc"]
_cache = {}


def _hash(gm, kind):
    return fm.Sha256() if kind == "sha256" else fm.MiMC(gm.BN254)


def _factory(gm, kind):
    return hashlib.sha256 if kind == "sha256" else (lambda: fm.MiMC(gm.BN254))


def _poly(gm, size, tag=0):
    rng = rng_for(0xF21, size, tag)
    return [int.from_bytes(rng.bytes(40), "big") % gm.BN254.r for _ in range(size)]


def _case(gm, kind, size):
    """(params, hash, polynomial, proof) of one size, computed once"""
    key = (kind, size)
    if key not in _cache:
        P, h, p = fm.Params(gm.BN254, size), _hash(gm, kind), _poly(gm, size)
        _cache[key] = (P, h, p, fm.prove(P, h, p))
    return _cache[key]


def _rev(i, m):
    return int(format(i, "0%db" % m)[::-1], 2) if m else 0


@pytest.mark.parametrize("kind", HASHES)
@pytest.mark.parametrize("size", SIZES)
def test_model_proof_passes_model_verifier(gm, kind, size):
    P, h, _, proof = _case(gm, kind, size)
    assert P.N == 8 * max(2, 1 << (size - 1).bit_length()) and len(proof.Rounds[0].Interactions) == P.nb_steps
    fm.verify(P, h, proof)
    for i, inter in enumerate(proof.Rounds[0].Interactions):
        assert inter[0].numLeaves == inter[1].numLeaves == P.N >> i
        assert sorted(len(x.ProofSet) for x in inter) == [2, P.nb_steps + 3 - i + 1]  # the leaf and log2(N >> i) siblings


@pytest.mark.parametrize("kind,size", [("sha256", s) for s in SIZES] + [("mimc", 2), ("mimc", 3), ("mimc", 4)])
def test_model_paths_equal_the_subtree_stack(gm, kind, size):
    """the model reads roots and paths off the levels; the reference pushes the leaves through its stack of subtrees twice a step"""
    P, h, p, proof = _case(gm, kind, size)
    lay, trees, _, _, _, _ = fm.layers(P, h, p)
    H = fm.H_of(h)
    rnd = proof.Rounds[0]
    si = fm.derive_queries_positions(_query_position(P, h, rnd, rnd.Evaluation), P.N, P.nb_steps)
    for i, inter in enumerate(rnd.Interactions):
        full = max(inter, key=lambda x: len(x.ProofSet))
        leaves = [P.marshal(v) for v in lay[i]]
        index = si[i]
        root, proof_set, _, num = mm.stack_tree(H, leaves, index)
        assert (root, proof_set, num) == (full.MerkleRoot, full.ProofSet, full.numLeaves)
        other = min(inter, key=lambda x: len(x.ProofSet))
        assert other.ProofSet == [leaves[index ^ 1], H(leaves[index])] and other.MerkleRoot == root


@pytest.mark.parametrize("kind", HASHES)
@pytest.mark.parametrize("size", SIZES)
def test_openings_claim_horner(gm, kind, size):
    P, h, p, proof = _case(gm, kind, size)
    tree = fm.layers(P, h, p)[1][0]
    for pos in [0, P.N // 2 - 1, P.N // 2, P.N - 1]:  # both branches of convertCanonicalSorted
        o = fm.open_(P, h, p, pos, tree)
        assert o.ClaimedValue == fm.horner(P, p, pow(P.gen, pos, P.r))
        assert o.index == fm.convert_canonical_sorted(pos, P.N) and o.numLeaves == P.N
        fm.verify_opening(P, h, pos, o, proof)
    with pytest.raises(ValueError, match=fm.ErrRangePosition):
        fm.open_(P, h, p, P.N)


@pytest.mark.parametrize("size", SIZES)
def test_query_positions_stay_in_the_fibre(gm, size):
    """the reference's fourth property: position i + 1 is where the square of the point at position i lies in the next layer"""
    P = fm.Params(gm.BN254, size)
    rng = rng_for(0xF22, size)
    for pos in [0, 1, P.N - 2, P.N - 1] + [int(v) for v in rng.integers(0, P.N, 12)]:
        si = fm.derive_queries_positions(pos, P.N, P.nb_steps)
        assert len(si) == P.nb_steps and si[0] == pos
        g, n = P.gen, P.N
        for i in range(P.nb_steps - 1):
            # the point at entry s of a sorted layer of size n: g^(s/2) for even s, g^(s/2 + n/2) for odd s
            point = lambda s, g, n: pow(g, s // 2 + (n // 2 if s % 2 else 0), P.r)
            assert pow(point(si[i], g, n), 2, P.r) == point(si[i + 1], g * g % P.r, n // 2)
            assert 0 <= si[i + 1] < n // 2
            g, n = g * g % P.r, n // 2


@pytest.mark.parametrize("size", SIZES)
def test_sorted_layer_is_one_gather_of_the_dif_output(gm, size):
    P, p = fm.Params(gm.BN254, size), _poly(gm, size, 1)
    q = ([v for v in p] + [0] * P.N)[:P.N]
    dif = fm.dif_fft(q, P.gen, P.r)
    two_pass = fm.sort(fm.bit_reverse(dif))
    m = P.N.bit_length() - 1
    assert two_pass == [dif[2 * _rev(j // 2, m - 1) + j % 2] for j in range(P.N)]
    assert fm.bit_reverse(dif) == [fm.horner(P, p, pow(P.gen, i, P.r)) for i in range(P.N)]


@pytest.mark.parametrize("size", SIZES)
def test_fused_fold_layout(gm, size):
    """lane j < s/4 reads the pairs at 2j and 2j + s/2, takes w^-(j 2^k) and w^-(j 2^k + N/4) from the table of the first domain
    and writes res[j], res[j + s/4] side by side: the same as fold, g <- g^2, sort"""
    P, p = fm.Params(gm.BN254, size), _poly(gm, size, 2)
    table = [pow(P.gen_inv, t, P.r) for t in range(P.N // 2)]
    rng = rng_for(0xF23, size)
    cur, g_inv = fm.sort(fm.evaluations(P, p)), P.gen_inv
    for k in range(P.nb_steps):
        x = [0, P.r - 1, int.from_bytes(rng.bytes(40), "big") % P.r][k % 3]
        res = fm.fold(cur, g_inv, x, P)
        s = len(cur)
        fused = [0] * (s // 2)
        for j in range(s // 4):
            for b, t in ((0, j << k), (1, (j << k) + P.N // 4)):
                assert t < P.N // 2
                lo, hi = cur[2 * j + b * (s // 2)], cur[2 * j + b * (s // 2) + 1]
                fused[2 * j + b] = ((lo - hi) * table[t] * x + lo + hi) * P.two_inv % P.r
        assert fused == fm.sort(res)
        cur, g_inv = fused, g_inv * g_inv % P.r
    assert len(cur) == 8


# ---- the package's host verifiers over the model's proofs
@pytest.mark.parametrize("kind", HASHES)
@pytest.mark.parametrize("size", SIZES)
def test_package_verifiers_accept_model_proofs(gm, kind, size):
    P, h, p, proof = _case(gm, kind, size)
    s = gm.fri.RADIX_2_FRI.New("bn254", size, _factory(gm, kind))
    assert (s.nbSteps, s.Cardinality) == (P.nb_steps, P.N) and gm.fri.GetRho() == gm.fri.rho == 8 and gm.fri.nbRounds == 1
    s.VerifyProofOfProximity(proof)
    pos = P.N // 2 + 1 if size > 2 else 3
    o = fm.open_(P, h, p, pos)
    s.VerifyOpening(pos, o, proof)
    for i in (0, 1, P.N // 2 - 1, P.N // 2, P.N - 1):
        assert gm.fri.convertCanonicalSorted(i, P.N) == fm.convert_canonical_sorted(i, P.N)
        assert gm.fri.deriveQueriesPositions(i, P.N, P.nb_steps) == fm.derive_queries_positions(i, P.N, P.nb_steps)


def _query_position(P, h, rnd, evaluation):
    """the first queried position of a round whose Evaluation is `evaluation`: the transcript replayed"""
    names = ["x%d" % i for i in range(P.nb_steps)] + ["s0"]
    fs = fm.Transcript(h, names)
    fs.bind(names[0], P.marshal(0))
    for i in range(P.nb_steps):
        fs.bind(names[i], rnd.Interactions[i][0].MerkleRoot)
        fs.compute(names[i])
    fs.bind("s0", P.marshal(evaluation))
    return int.from_bytes(fs.compute("s0"), "big") % P.N


def _flip(b):
    return b[:-1] + bytes([b[-1] ^ 1])  # the lowest bit: still canonical


@pytest.mark.parametrize("kind", HASHES)
@pytest.mark.parametrize("size", SIZES)
def test_package_verifiers_reject_tampering(gm, kind, size):
    P, h, p, proof = _case(gm, kind, size)
    s = gm.fri.RADIX_2_FRI.New("bn254", size, _factory(gm, kind))
    errs = (gm.fri.ErrMerklePath, gm.fri.ErrProximityTestFolding, gm.fri.ErrMerkleRoot)
    assert errs == (fm.ErrMerklePath, fm.ErrProximityTestFolding, fm.ErrMerkleRoot)
    # a leaf of the first step (a later step's leaf is held against the fold of the step before it first, fri.go:617-641), and a
    # sibling of the last step's full path
    tampered = []
    for b in (0, 1):
        bad = copy.deepcopy(proof)
        ps = bad.Rounds[0].Interactions[0][b].ProofSet
        ps[0] = _flip(ps[0])
        tampered.append(bad)
    bad = copy.deepcopy(proof)
    ps = max(bad.Rounds[0].Interactions[P.nb_steps - 1], key=lambda x: len(x.ProofSet)).ProofSet
    ps[-1] = _flip(ps[-1])
    tampered.append(bad)
    for bad in tampered:
        for check in (s.VerifyProofOfProximity, lambda x: fm.verify(P, h, x)):
            with pytest.raises(ValueError) as e:
                check(bad)
            assert str(e.value) == fm.ErrMerklePath
    # The verifier derives the queries from the Evaluation, so a changed one usually moves them and a path fails first. The
    # folding check itself (the last transition against the Evaluation, fri.go:649-667) is reached by a change that leaves the
    # queries where they were: Evaluation + k for the first k whose seed gives the same position modulo N.
    rnd = proof.Rounds[0]
    want = _query_position(P, h, rnd, rnd.Evaluation)
    k = next(k for k in range(1, 40 * P.N) if _query_position(P, h, rnd, (rnd.Evaluation + k) % P.r) == want)
    bad = copy.deepcopy(proof)
    bad.Rounds[0].Evaluation = (rnd.Evaluation + k) % P.r
    for check in (s.VerifyProofOfProximity, lambda x: fm.verify(P, h, x)):
        with pytest.raises(ValueError) as e:
            check(bad)
        assert str(e.value) == fm.ErrProximityTestFolding
    pos = 5
    o = fm.open_(P, h, p, pos)
    with pytest.raises(ValueError) as e:
        s.VerifyOpening(pos + 1, o, proof)
    assert str(e.value) == fm.ErrMerklePath
    other = fm.prove(P, h, _poly(gm, size, 7))
    with pytest.raises(ValueError) as e:
        s.VerifyOpening(pos, o, other)
    assert str(e.value) == fm.ErrMerkleRoot
    s.VerifyOpening(pos, o, proof)


def test_new_refuses_what_the_reference_cannot_verify(gm):
    for size in (0, 1):
        with pytest.raises(ValueError, match="size at least 2"):
            gm.fri.RADIX_2_FRI.New("bn254", size, hashlib.sha256)
    with pytest.raises(ValueError, match="root of unity"):
        gm.fri.RADIX_2_FRI.New("bn254", 1 << 26, hashlib.sha256)
    s = gm.fri.RADIX_2_FRI.New("bn254", 4, hashlib.sha256)
    with pytest.raises(ValueError) as e:
        s.Open(None, s.Cardinality)
    assert str(e.value) == "the asked opening position is out of range"
    # the device prover commits with MiMC trees: any other hash is refused before the device is looked for
    for factory in (hashlib.sha256, lambda: gm.mimc.NewMiMC("bls12_381"), lambda: gm.mimc.NewMiMC("bn254", byte_order="little")):
        with pytest.raises(ValueError, match="MiMC"):
            gm.fri.RADIX_2_FRI.New("bn254", 4, factory).Commit([[0, 0, 0, 0]])
