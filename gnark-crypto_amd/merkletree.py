"""accumulator/merkletree (tree.go, verify.go) over fr/mimc, built on the device: DeviceTree hashes n leaves of leaf_len
elements each and every level above them in HBM (gmsm_merkle_new), answers Root() from the host copy of the root and
Prove(indices) with one gather launch for all paths (gmsm_merkle_prove). Proof sets are the reference's, in bytes: proofSet[0]
is the leaf's data (its elements, canonical big-endian, one after the other), the rest the siblings' sums bottom up. In this
version of the reference leafSum(data) = H(data) and nodeSum(a, b) = H(a || b): the prefixes are commented out (tree.go:92-105).
VerifyProof is the reference's verifier on the host, over any hash object with Reset / Write / Sum (mimc.NewMiMC)."""
import ctypes

import numpy as np

from . import _lib
from .polynomial import _check, _curve, _gid, _ptr, to_int


def _bytes(c, limbs):
    return to_int(c, limbs).to_bytes(8 * c.fr_limbs, "big")


class DeviceTree:
    def __init__(self, curve, leaves=None, d_leaves=None, n=None, leaf_len=1, keep_leaves=True, stream=0):
        """leaves: (n, leaf_len, fr_limbs) Montgomery limbs on the host, or d_leaves: a device pointer to as many with n given."""
        c = self.curve = _curve(curve)
        host = None
        if leaves is not None:
            host = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, int(leaf_len), c.fr_limbs)
            n = host.shape[0] if n is None else n
            if n != host.shape[0]:
                raise ValueError("expected %d leaves, got %d" % (n, host.shape[0]))
        handle = ctypes.c_uint64(0)
        _check(_lib.load().gmsm_merkle_new(_gid(c), None if host is None else _ptr(host), d_leaves, int(n or 0), int(leaf_len), int(bool(keep_leaves)),
                                           stream or None, ctypes.byref(handle)))
        self.handle = handle.value
        nn, ll, depth = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint(0)
        _check(_lib.load().gmsm_merkle_info(self.handle, ctypes.byref(nn), ctypes.byref(ll), ctypes.byref(depth)))
        self.n, self.leaf_len, self.depth, self.keep_leaves = nn.value, ll.value, depth.value, bool(keep_leaves)

    def NumLeaves(self):
        return self.n

    def root_limbs(self):
        out = np.zeros(self.curve.fr_limbs, dtype=np.uint64)
        _check(_lib.load().gmsm_merkle_root(self.handle, _ptr(out)))
        return out

    def Root(self):
        return _bytes(self.curve, self.root_limbs())

    def prove_limbs(self, indices, with_leaves=None):
        """(leaves or None, siblings (k, depth, fr_limbs), counts (k,)): the paths as the C ABI returns them"""
        c = self.curve
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        k = len(idx)
        with_leaves = self.keep_leaves if with_leaves is None else with_leaves
        leaves = np.zeros((k, self.leaf_len, c.fr_limbs), dtype=np.uint64) if with_leaves else None
        sibs = np.zeros((k, self.depth, c.fr_limbs), dtype=np.uint64)
        counts = np.zeros(k, dtype=np.uint32)
        _check(_lib.load().gmsm_merkle_prove(self.handle, _ptr(idx), k, None if leaves is None else _ptr(leaves), _ptr(sibs), _ptr(counts)))
        return leaves, sibs, counts

    def Prove(self, indices, leaf_data=None):
        """[(merkleRoot, proofSet, proofIndex, numLeaves)] for the indices, as (*Tree).Prove returns them. A tree built
        without keep_leaves needs leaf_data: the leaves at the indices, (k, leaf_len, fr_limbs) Montgomery limbs."""
        c = self.curve
        if not self.keep_leaves and leaf_data is None:
            raise ValueError("the tree was built without keep_leaves: give the leaves' data (proofSet[0]) as leaf_data")
        leaves, sibs, counts = self.prove_limbs(indices, with_leaves=leaf_data is None)
        if leaf_data is not None:
            leaves = np.ascontiguousarray(leaf_data, dtype=np.uint64).reshape(len(counts), self.leaf_len, c.fr_limbs)
        root = self.Root()
        out = []
        for j, index in enumerate(np.asarray(indices, dtype=np.uint64).reshape(-1)):
            proof = [b"".join(_bytes(c, e) for e in leaves[j])] + [_bytes(c, sibs[j, l]) for l in range(int(counts[j]))]
            out.append((root, proof, int(index), self.n))
        return out

    def Release(self):
        _check(_lib.load().gmsm_merkle_release(self.handle))


def _sum(h, *data):
    h.Reset()
    for d in data:
        h.Write(d)
    return h.Sum(b"")


def VerifyProof(h, merkleRoot, proofSet, proofIndex, numLeaves):
    """verify.go:31-137: whether proofSet[0] is the data of leaf proofIndex of a tree of numLeaves leaves with this root."""
    if merkleRoot is None or proofIndex >= numLeaves:
        return False
    height = 0
    if len(proofSet) <= height:
        return False
    acc = _sum(h, proofSet[height])
    height += 1
    stableEnd = proofIndex
    while True:
        start = (proofIndex >> height) << height
        end = start + (1 << height) - 1
        if end >= numLeaves:
            break
        stableEnd = end
        if len(proofSet) <= height:
            return False
        if proofIndex - start < 1 << (height - 1):
            acc = _sum(h, acc, proofSet[height])
        else:
            acc = _sum(h, proofSet[height], acc)
        height += 1
    if stableEnd != numLeaves - 1:
        if len(proofSet) <= height:
            return False
        acc = _sum(h, acc, proofSet[height])
        height += 1
    while height < len(proofSet):
        acc = _sum(h, proofSet[height], acc)
        height += 1
    return acc == bytes(merkleRoot)
