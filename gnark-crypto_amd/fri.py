"""fr/fri (ecc/<curve>/fr/fri/fri.go) over libgmsm.so: RADIX_2_FRI with rho = 8 and nbRounds = 1.

The prover runs on the device (gmsm_fri_*): the layers and their Merkle trees stay in HBM from the first FFT to the last path, a
tree is built once per step instead of twice, and only roots, the Evaluation and the queried paths come back. The device tree is
MiMC, so the prover needs hash_factory to make a big-endian mimc.MiMC of the same curve; any other hash is refused. The two
verifiers are host code of the size of a proof, over any hash: hash_factory() may return an object with Reset / Write / Sum
(mimc.NewMiMC) or with update / digest (hashlib.sha256, the reference's own test hash).

Polynomials are Montgomery limbs, (len, fr_limbs) uint64 on the host or a device pointer d_p with n elements; more than
Cardinality coefficients are cut, as Go's copy does. Proofs carry the reference's field names and byte contents; the two
fr.Element fields (Round.Evaluation, OpeningProof.ClaimedValue) are Python integers, the element's value.
Beyond the reference: Commit(p) returns an Oracle, which BuildProofOfProximity and Open take in place of p, so that an opening
after a proof costs one gather instead of a second FFT and tree."""
import ctypes

import numpy as np

from . import _lib, fiatshamir, merkletree, mimc
from .polynomial import _check, _curve, _elems, _ptr, from_int, to_int

rho = 8
nbRounds = 1

ErrLowDegree = "the fully folded polynomial in not of degree 1"
ErrProximityTestFolding = "one round of interaction failed"
ErrOddSize = "the size should be even"
ErrMerkleRoot = "merkle roots of the opening and the proof of proximity don't coincide"
ErrMerklePath = "merkle path proof is wrong"
ErrRangePosition = "the asked opening position is out of range"


def GetRho():
    return rho


class MerkleProof:
    def __init__(self, MerkleRoot=None, ProofSet=None, numLeaves=0):
        self.MerkleRoot, self.ProofSet, self.numLeaves = MerkleRoot, ProofSet if ProofSet is not None else [], numLeaves


class OpeningProof:
    def __init__(self, merkleRoot=None, ProofSet=None, numLeaves=0, index=0, ClaimedValue=0):
        self.merkleRoot, self.ProofSet, self.numLeaves, self.index = merkleRoot, ProofSet if ProofSet is not None else [], numLeaves, index
        self.ClaimedValue = ClaimedValue


class Round:
    def __init__(self, Interactions=None, Evaluation=0):
        self.Interactions, self.Evaluation = Interactions if Interactions is not None else [], Evaluation


class ProofOfProximity:
    def __init__(self, ID=None, Rounds=None):
        self.ID, self.Rounds = ID, Rounds if Rounds is not None else []


def convertCanonicalSorted(i, n):
    """the entry of a sorted polynomial of size n that holds entry i of the canonical one (fri.go:202-212)"""
    if i < n // 2:
        return 2 * i
    return n - 2 * (n - (i + 1)) - 1


def deriveQueriesPositions(pos, size, nbSteps):
    """fri.go:221-233: the queried entry of every step's sorted layer, from the first one"""
    s, res = size // 2, [pos]
    for _ in range(1, nbSteps):
        t = (res[-1] - res[-1] % 2) // 2
        res.append(convertCanonicalSorted(t, s))
        s //= 2
    return res


class _Hash:
    """Reset / Write / Sum for the Merkle verifier and update / digest for the transcript over whatever hash_factory makes"""

    def __init__(self, factory):
        self.factory = factory
        self.Reset()

    def Reset(self):
        self.h = self.factory()

    def Write(self, p):
        return self.h.Write(p) if hasattr(self.h, "Write") else self.h.update(p)

    def Sum(self, b=b""):
        return bytes(b) + bytes(self.h.Sum(b"") if hasattr(self.h, "Sum") else self.h.digest())

    update = Write

    def digest(self):
        return self.Sum()


class Oracle:
    """A FRI oracle on the device (gmsm_fri_commit): the sorted layers built so far and one MiMC tree over each."""

    def __init__(self, curve, domain, p=None, d_p=None, n=None, stream=0):
        c = self.curve = _curve(curve)
        host = None
        if p is not None:
            host = _elems(c, p)[:domain.Cardinality]
            n = len(host)
        handle = ctypes.c_uint64(0)
        _check(_lib.load().gmsm_fri_commit(domain.handle, None if host is None else _ptr(host), d_p, min(int(n or 0), domain.Cardinality),
                                           stream or None, ctypes.byref(handle)))
        self.handle = handle.value
        card, steps = ctypes.c_uint64(0), ctypes.c_uint(0)
        _check(_lib.load().gmsm_fri_info(self.handle, ctypes.byref(card), ctypes.byref(steps), None))
        self.Cardinality, self.nbSteps = int(card.value), int(steps.value)
        self.log2n = self.Cardinality.bit_length() - 1

    def folds_done(self):
        done = ctypes.c_uint(0)
        _check(_lib.load().gmsm_fri_info(self.handle, None, None, ctypes.byref(done)))
        return int(done.value)

    def root_limbs(self, step):
        out = np.zeros(self.curve.fr_limbs, dtype=np.uint64)
        _check(_lib.load().gmsm_fri_root(self.handle, int(step), _ptr(out)))
        return out

    def Root(self, step):
        return merkletree._bytes(self.curve, self.root_limbs(step))

    def fold(self, xi):
        """one fold with the challenge xi (limbs): the new layer's root, or the Evaluation after the last fold (limbs)"""
        out = np.zeros(self.curve.fr_limbs, dtype=np.uint64)
        _check(_lib.load().gmsm_fri_fold(self.handle, _ptr(_elems(self.curve, xi, 1)), _ptr(out)))
        return out

    def layer(self, step):
        """the sorted evaluations of a layer, (Cardinality >> step, fr_limbs)"""
        out = np.zeros((self.Cardinality >> int(step), self.curve.fr_limbs), dtype=np.uint64)
        _check(_lib.load().gmsm_fri_layer(self.handle, int(step), _ptr(out), None))
        return out

    def layer_device(self, step, d_out):
        _check(_lib.load().gmsm_fri_layer(self.handle, int(step), None, d_out))

    def query_limbs(self, positions):
        """(pairs (k, 2, fr_limbs), leaf sums (k, fr_limbs), siblings (k, log2 N, fr_limbs), counts (k,)) as the C ABI returns them"""
        c = self.curve
        pos = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
        k = len(pos)
        pairs = np.zeros((k, 2, c.fr_limbs), dtype=np.uint64)
        sums = np.zeros((k, c.fr_limbs), dtype=np.uint64)
        sibs = np.zeros((k, self.log2n, c.fr_limbs), dtype=np.uint64)
        counts = np.zeros(k, dtype=np.uint32)
        _check(_lib.load().gmsm_fri_query(self.handle, _ptr(pos), k, _ptr(pairs), _ptr(sums), _ptr(sibs), _ptr(counts)))
        return pairs, sums, sibs, counts

    def Release(self):
        _check(_lib.load().gmsm_fri_release(self.handle))


class radixTwoFri:
    def __init__(self, curve, size, hash_factory):
        c = self.curve = _curve(curve)
        size = int(size)
        if size < 2:
            raise ValueError("fri: size = %d: the protocol needs a polynomial of size at least 2" % size)
        n = 1 << (size - 1).bit_length()  # ecc.NextPowerOfTwo
        self.nbSteps = n.bit_length() - 1
        self.Cardinality = n * rho
        if self.Cardinality.bit_length() - 1 > c.fr_max_order:
            raise ValueError("m is too big: the required root of unity does not exist")
        self.hash_factory = hash_factory
        self.bs = 8 * c.fr_limbs
        gen = pow(c.fr_root_of_unity, 1 << (c.fr_max_order - (self.Cardinality.bit_length() - 1)), c.r)
        self.GeneratorInv = pow(gen, -1, c.r)
        self.twoInv = pow(2, -1, c.r)
        self._domain = None

    # ---- the prover, on the device
    def _device_domain(self):
        h = self.hash_factory()
        if not (isinstance(h, mimc.MiMC) and h.byte_order == "big" and h.curve is self.curve):
            raise ValueError("fri: the device prover commits with MiMC trees: hash_factory must make a big-endian mimc.MiMC of %s"
                             % self.curve.name)
        if self._domain is None:
            from . import fft
            self._domain = fft.NewDomain(self.curve, self.Cardinality)
        return self._domain

    def Commit(self, p=None, d_p=None, n=None, stream=0):
        return Oracle(self.curve, self._device_domain(), p, d_p, n, stream)

    def _oracle(self, p, d_p, n, stream):
        """(oracle, whether it is ours to release)"""
        if isinstance(p, Oracle):
            if p.Cardinality != self.Cardinality or p.curve is not self.curve:
                raise ValueError("fri: the oracle was committed over another domain")
            return p, False
        return self.Commit(p, d_p, n, stream), True

    def _marshal(self, v):
        return int(v).to_bytes(self.bs, "big")

    def _bytes(self, limbs):
        return self._marshal(to_int(self.curve, limbs))

    def _transcript(self):
        xis = ["x%d" % i for i in range(self.nbSteps)] + ["s0"]
        return xis, fiatshamir.NewTranscript(lambda: _Hash(self.hash_factory), *xis)

    def _positions(self, fs, xis, evaluation):
        fs.Bind(xis[self.nbSteps], self._marshal(evaluation))
        seed = fs.ComputeChallenge(xis[self.nbSteps])
        return deriveQueriesPositions(int.from_bytes(seed, "big") % self.Cardinality, self.Cardinality, self.nbSteps)

    def BuildProofOfProximity(self, p=None, d_p=None, n=None, stream=0):
        c = self.curve
        o, ours = self._oracle(p, d_p, n, stream)
        try:
            if o.folds_done():
                raise ValueError("fri: the oracle is folded already: a proof of proximity starts from a fresh Commit")
            xis, fs = self._transcript()
            fs.Bind(xis[0], self._marshal(0))  # the salt of round 0
            roots, out = [], None
            for i in range(self.nbSteps):
                roots.append(o.Root(i))
                fs.Bind(xis[i], roots[i])
                xi = int.from_bytes(fs.ComputeChallenge(xis[i]), "big") % c.r
                out = o.fold(from_int(c, xi))
            res = Round(Evaluation=to_int(c, out))
            si = self._positions(fs, xis, res.Evaluation)
            pairs, sums, sibs, counts = o.query_limbs(si)
            for i in range(self.nbSteps):
                b = si[i] % 2
                full = [self._bytes(pairs[i, b])] + [self._bytes(sibs[i, l]) for l in range(int(counts[i]))]
                inter = [None, None]
                inter[b] = MerkleProof(roots[i], full, self.Cardinality >> i)
                inter[1 - b] = MerkleProof(roots[i], [self._bytes(pairs[i, 1 - b]), self._bytes(sums[i])], self.Cardinality >> i)
                res.Interactions.append(inter)
            return ProofOfProximity(Rounds=[res])
        finally:
            if ours:
                o.Release()

    def Open(self, p=None, position=0, d_p=None, n=None, stream=0):
        position = int(position)
        if position >= self.Cardinality:
            raise ValueError(ErrRangePosition)
        o, ours = self._oracle(p, d_p, n, stream)
        try:
            pos = convertCanonicalSorted(position, self.Cardinality)
            pairs, _, sibs, counts = o.query_limbs([pos])
            leaf = pairs[0, pos % 2]
            proof = [self._bytes(leaf)] + [self._bytes(sibs[0, l]) for l in range(int(counts[0]))]
            return OpeningProof(o.Root(0), proof, self.Cardinality, pos, to_int(self.curve, leaf))
        finally:
            if ours:
                o.Release()

    # ---- the verifiers, on the host
    def VerifyOpening(self, position, openingProof, pp):
        first = pp.Rounds[0].Interactions[0]
        full = 0 if len(first[0].ProofSet) > len(first[1].ProofSet) else 1
        if bytes(openingProof.merkleRoot) != bytes(first[full].MerkleRoot):
            raise ValueError(ErrMerkleRoot)
        pos = convertCanonicalSorted(int(position), self.Cardinality)
        if not merkletree.VerifyProof(_Hash(self.hash_factory), openingProof.merkleRoot, openingProof.ProofSet, pos, openingProof.numLeaves):
            raise ValueError(ErrMerklePath)

    def _fold_pair(self, inter, ginv, xi):
        r = self.curve.r
        lo, hi = (int.from_bytes(inter[b].ProofSet[0], "big") % r for b in (0, 1))
        return ((lo - hi) * ginv * xi + lo + hi) * self.twoInv % r

    def _verify_round(self, salt, proof):
        r = self.curve.r
        h = _Hash(self.hash_factory)
        xis, fs = self._transcript()
        fs.Bind(xis[0], self._marshal(salt))
        xi = []
        for i in range(self.nbSteps):
            fs.Bind(xis[i], proof.Interactions[i][0].MerkleRoot)
            xi.append(int.from_bytes(fs.ComputeChallenge(xis[i]), "big") % r)
        si = self._positions(fs, xis, proof.Evaluation)
        acc = self.GeneratorInv
        for i in range(self.nbSteps):
            inter = proof.Interactions[i]
            b = si[i] % 2
            if not merkletree.VerifyProof(h, inter[b].MerkleRoot, inter[b].ProofSet, si[i], inter[b].numLeaves):
                raise ValueError(ErrMerklePath)
            other = list(inter[1 - b].ProofSet[:2]) + list(inter[b].ProofSet[2:])
            if not merkletree.VerifyProof(h, inter[1 - b].MerkleRoot, other, si[i] + 1 - 2 * b, inter[1 - b].numLeaves):
                raise ValueError(ErrMerklePath)
            if i < self.nbSteps - 1:
                fo = self._fold_pair(inter, pow(acc, si[i] // 2, r), xi[i])
                nxt = proof.Interactions[i + 1][si[i + 1] % 2].ProofSet[0]
                if fo != int.from_bytes(nxt, "big") % r:
                    raise ValueError(ErrProximityTestFolding)
                acc = acc * acc % r
        last = self.nbSteps - 1
        fo = self._fold_pair(proof.Interactions[last], pow(acc, si[last] // 2, r), xi[last])
        if fo != int(proof.Evaluation) % r:
            raise ValueError(ErrProximityTestFolding)

    def VerifyProofOfProximity(self, proof):
        for i in range(nbRounds):
            self._verify_round(i, proof.Rounds[i])

    def Release(self):
        if self._domain is not None:
            self._domain.release()
            self._domain = None


class IOPP(int):
    """fri.IOPP: RADIX_2_FRI.New(curve, size, hash_factory)"""

    def New(self, curve, size, hash_factory):
        if self != 0:
            raise ValueError("iopp name is not recognized")
        return radixTwoFri(curve, size, hash_factory)


RADIX_2_FRI = IOPP(0)
