"""Big-int model of the reference's fr/fri (ecc/<curve>/fr/fri/fri.go), independent of the library: sort, convertCanonicalSorted,
deriveQueriesPositions, foldPolynomialLagrangeBasis, the prover, Open and both verifiers, over any hash object with Reset / Write /
Sum. Trees come from mimc_model: each step's tree is built once, level by level (mimc_model.levels), and roots and paths are read
off it; tests/test_fri_model.py holds every path against the reference's subtree stack (mimc_model.stack_tree). The transcript
is fiat-shamir/transcript.go restated. Field elements are integers, proofs carry
the reference's field names (Evaluation and ClaimedValue as integers)."""
import hashlib
from types import SimpleNamespace as NS

import mimc_model as mm

RHO = 8
NB_ROUNDS = 1

ErrProximityTestFolding = "one round of interaction failed"
ErrMerkleRoot = "merkle roots of the opening and the proof of proximity don't coincide"
ErrMerklePath = "merkle path proof is wrong"
ErrRangePosition = "the asked opening position is out of range"


class Sha256:
    """hashlib.sha256 as a Go hash.Hash"""

    def __init__(self):
        self.Reset()

    def Reset(self):
        self.h = hashlib.sha256()

    def Write(self, p):
        self.h.update(p)

    def Sum(self, b=b""):
        return b + self.h.digest()


class MiMC(mm.Hash):
    """the MiMC model as the transcript needs it: an input shorter than one block is left-padded with zeros (mimc.go:102-110)"""

    def Write(self, p):
        if 0 < len(p) < self.bs:
            p = bytes(self.bs - len(p)) + p
        mm.Hash.Write(self, p)


def H_of(h):
    """leafSum / nodeSum over a hash object: H(data), H(a, b) = the hash of the concatenation"""
    def H(*data):
        h.Reset()
        for d in data:
            h.Write(d)
        return h.Sum(b"")
    return H


class Params:
    """newRadixTwoFri (fri.go:178-197) for a curve object with .r, .fr_limbs, .fr_root_of_unity, .fr_max_order"""

    def __init__(self, curve, size):
        n = 1
        while n < size:
            n *= 2
        self.curve, self.r, self.bs = curve, curve.r, 8 * curve.fr_limbs
        self.nb_steps = n.bit_length() - 1
        self.N = n * RHO
        self.gen = pow(curve.fr_root_of_unity, 1 << (curve.fr_max_order - (self.N.bit_length() - 1)), self.r)
        self.gen_inv = pow(self.gen, -1, self.r)
        self.two_inv = pow(2, -1, self.r)

    def marshal(self, v):
        return (v % self.r).to_bytes(self.bs, "big")

    def set_bytes(self, b):
        return int.from_bytes(b, "big") % self.r


def convert_canonical_sorted(i, n):
    if i < n // 2:
        return 2 * i
    l = 2 * (n - (i + 1))
    return n - l - 1


def derive_queries_positions(pos, size, nb_steps):
    s, res = size // 2, [0] * nb_steps
    res[0] = pos
    for i in range(1, nb_steps):
        t = (res[i - 1] - (res[i - 1] % 2)) // 2
        res[i] = convert_canonical_sorted(t, s)
        s //= 2
    return res


def sort(evaluations):
    n = len(evaluations) // 2
    q = [0] * len(evaluations)
    for i in range(n):
        q[2 * i], q[2 * i + 1] = evaluations[i], evaluations[i + n]
    return q


def fold(p_sorted, g_inv, x, P):
    """foldPolynomialLagrangeBasis (fri.go:332-355), the serial acc *= gInv chain as it stands there"""
    r, acc, res = P.r, 1, []
    for i in range(len(p_sorted) // 2):
        p1 = p_sorted[2 * i] + p_sorted[2 * i + 1]
        p2 = (p_sorted[2 * i] - p_sorted[2 * i + 1]) * acc
        res.append((p2 * x + p1) * P.two_inv % r)
        acc = acc * g_inv % r
    return res


def dif_fft(a, g, r):
    """(*Domain).FFT(a, fft.DIF): natural in, bit-reversed out; radix-2 Gentleman-Sande butterflies"""
    a, n = list(a), len(a)
    half, w = n // 2, g
    while half >= 1:
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * w % r
        for start in range(0, n, 2 * half):
            for j in range(half):
                x, y = a[start + j], a[start + j + half]
                a[start + j], a[start + j + half] = (x + y) % r, (x - y) * tw[j] % r
        w, half = w * w % r, half // 2
    return a


def bit_reverse(a):
    n = len(a)
    m = n.bit_length() - 1
    return [a[int(format(i, "0%db" % m)[::-1], 2) if m else 0] for i in range(n)]


def evaluations(P, p):
    """copy(_p, p); FFT(DIF); BitReverse: p on the domain, in natural order"""
    q = ([v % P.r for v in p] + [0] * P.N)[:P.N]
    return bit_reverse(dif_fft(q, P.gen, P.r))


def horner(P, p, x):
    acc = 0
    for v in reversed(list(p)[:P.N]):
        acc = (acc * x + v) % P.r
    return acc


class Transcript:
    """fiat-shamir/transcript.go over one hash object, reset for every challenge"""

    def __init__(self, h, names):
        self.h, self.pos = h, {name: i for i, name in enumerate(names)}
        self.bindings, self.values, self.previous = {name: [] for name in names}, {}, None

    def bind(self, name, value):
        assert name in self.pos and name not in self.values
        self.bindings[name].append(bytes(value))

    def compute(self, name):
        if name in self.values:
            return self.values[name]
        self.h.Reset()
        self.h.Write(name.encode())
        if self.pos[name] != 0:
            assert self.previous is not None and self.previous[0] == self.pos[name] - 1
            self.h.Write(self.previous[1])
        for b in self.bindings[name]:
            self.h.Write(b)
        v = self.h.Sum(b"")
        self.values[name], self.previous = v, (self.pos[name], v)
        return v


def _names(P):
    return ["x%d" % i for i in range(P.nb_steps)] + ["s0"]


def _positions(P, fs, names, evaluation):
    fs.bind(names[P.nb_steps], P.marshal(evaluation))
    seed = fs.compute(names[P.nb_steps])
    return derive_queries_positions(int.from_bytes(seed, "big") % P.N, P.N, P.nb_steps)


def layers(P, h, p, challenges=None):
    """(the sorted layer of every step, the levels of every step's tree, the challenges, the Evaluation, the transcript, its
    names). challenges: fold with these instead of deriving them; h = None skips every hash and needs them"""
    names = _names(P)
    fs = Transcript(h, names) if h is not None else None
    if fs:
        fs.bind(names[0], P.marshal(0))
    cur, g_inv = evaluations(P, p), P.gen_inv
    lay, trees, xs = [], [], []
    for i in range(P.nb_steps):
        lay.append(sort(cur))
        if fs:
            trees.append(mm.levels(H_of(h), [P.marshal(v) for v in lay[i]]))
            fs.bind(names[i], trees[i][-1][0])
            derived = P.set_bytes(fs.compute(names[i]))
        xs.append(challenges[i] if challenges is not None else derived)
        cur = fold(lay[i], g_inv, xs[i], P)
        g_inv = g_inv * g_inv % P.r
    return lay, trees, xs, cur[0], fs, names


def prove(P, h, p, pre=None):
    """BuildProofOfProximity (fri.go:361-520). pre: what layers(P, h, p) returned, when the caller has it"""
    lay, trees, _, evaluation, fs, names = pre if pre is not None else layers(P, h, p)
    res = NS(Interactions=[], Evaluation=evaluation)
    si = _positions(P, fs, names, evaluation)
    H = H_of(h)
    for i in range(P.nb_steps):
        leaves = [P.marshal(v) for v in lay[i]]
        mr, proof_set, _, num = mm.level_proof(trees[i], leaves, si[i])
        c = si[i] % 2
        inter = [None, None]
        inter[c] = NS(MerkleRoot=mr, ProofSet=proof_set, numLeaves=num)
        inter[1 - c] = NS(MerkleRoot=mr, ProofSet=[leaves[si[i] + 1 - 2 * c], H(proof_set[0])], numLeaves=num)
        res.Interactions.append(inter)
    return NS(ID=None, Rounds=[res])


def open_(P, h, p, position, tree=None):
    """Open (fri.go:249-284). tree: the levels over the first sorted layer when the caller has them (several openings of one p)"""
    if position >= P.N:
        raise ValueError(ErrRangePosition)
    q = sort(evaluations(P, p))
    pos = convert_canonical_sorted(position, len(q))
    leaves = [P.marshal(v) for v in q]
    root, proof_set, index, num = mm.level_proof(tree, leaves, pos) if tree is not None else mm.stack_tree(H_of(h), leaves, pos)
    return NS(merkleRoot=root, ProofSet=proof_set, numLeaves=num, index=index, ClaimedValue=P.set_bytes(proof_set[0]))


def verify_opening(P, h, position, opening, pp):
    first = pp.Rounds[0].Interactions[0]
    full = 0 if len(first[0].ProofSet) > len(first[1].ProofSet) else 1
    if opening.merkleRoot != first[full].MerkleRoot:
        raise ValueError(ErrMerkleRoot)
    pos = convert_canonical_sorted(position, P.N)
    if not mm.verify_proof(H_of(h), opening.merkleRoot, opening.ProofSet, pos, opening.numLeaves):
        raise ValueError(ErrMerklePath)


def verify(P, h, proof):
    """VerifyProofOfProximity (fri.go:524-687)"""
    r, H = P.r, H_of(h)
    rnd = proof.Rounds[0]
    names = _names(P)
    fs = Transcript(h, names)
    fs.bind(names[0], P.marshal(0))
    xi = []
    for i in range(P.nb_steps):
        fs.bind(names[i], rnd.Interactions[i][0].MerkleRoot)
        xi.append(P.set_bytes(fs.compute(names[i])))
    si = _positions(P, fs, names, rnd.Evaluation)
    acc = P.gen_inv

    def folded(i, ginv):
        lo, hi = (P.set_bytes(rnd.Interactions[i][b].ProofSet[0]) for b in (0, 1))
        return ((lo - hi) * ginv * xi[i] + lo + hi) * P.two_inv % r

    for i in range(P.nb_steps):
        inter, c = rnd.Interactions[i], si[i] % 2
        if not mm.verify_proof(H, inter[c].MerkleRoot, inter[c].ProofSet, si[i], inter[c].numLeaves):
            raise ValueError(ErrMerklePath)
        other = inter[1 - c].ProofSet[:2] + inter[c].ProofSet[2:]
        if not mm.verify_proof(H, inter[1 - c].MerkleRoot, other, si[i] + 1 - 2 * c, inter[1 - c].numLeaves):
            raise ValueError(ErrMerklePath)
        if i < P.nb_steps - 1:
            if folded(i, pow(acc, si[i] // 2, r)) != P.set_bytes(rnd.Interactions[i + 1][si[i + 1] % 2].ProofSet[0]):
                raise ValueError(ErrProximityTestFolding)
            acc = acc * acc % r
    last = P.nb_steps - 1
    if folded(last, pow(acc, si[last] // 2, r)) != rnd.Evaluation % r:
        raise ValueError(ErrProximityTestFolding)
