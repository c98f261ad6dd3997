"""Big-int model of the reference's MiMC (ecc/<curve>/fr/mimc/mimc.go) and of accumulator/merkletree over it, independent of the
library and of tools/gen_params.py: its own legacy Keccak-256, the constants' recipe, the Miyaguchi-Preneel loop, the
reference's subtree-stack tree restated (tree.go), the level-by-level tree the device builds, and the verifier (verify.go)."""

ROUNDS = {"bn254": 110, "bls12_381": 111, "bw6_761": 163}
M64 = (1 << 64) - 1


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def _round_constants():
    out, lfsr = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if lfsr & 1:
                rc |= 1 << ((1 << j) - 1)
            lfsr = ((lfsr << 1) ^ 0x171) if lfsr & 0x80 else lfsr << 1
        out.append(rc)
    return out


def _rotations():
    rot, (x, y) = {(0, 0): 0}, (1, 0)
    for t in range(24):
        rot[x, y] = (t + 1) * (t + 2) // 2 % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC, ROT = _round_constants(), _rotations()


def keccak_f(s):
    """Keccak-f[1600] on the 25 lanes s[x + 5 y]"""
    for rc in RC:
        c = [s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        s = [s[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(s[x + 5 * y], ROT[x, y])
        s = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & M64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        s[0] ^= rc
    return s


def keccak256(data):
    """legacy Keccak-256 (sha3.NewLegacyKeccak256): rate 136, padding 0x01 .. 0x80 - not hashlib.sha3_256, which pads with 0x06"""
    rate = 136
    msg = bytearray(data) + b"\x01" + bytes(-(len(data) + 1) % rate)
    msg[-1] |= 0x80
    s = [0] * 25
    for off in range(0, len(msg), rate):
        for i in range(rate // 8):
            s[i] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        s = keccak_f(s)
    return b"".join(v.to_bytes(8, "little") for v in s[:4])


_constants = {}


def constants(curve):
    """initConstants (mimc.go:176-191) for a curve object with .name and .r"""
    if curve.name not in _constants:
        rnd, out = keccak256(b"seed"), []
        for _ in range(ROUNDS[curve.name]):
            rnd = keccak256(rnd)
            out.append(int.from_bytes(rnd, "big") % curve.r)
        _constants[curve.name] = out
    return _constants[curve.name]


def mimc(curve, elems, h=0):
    """checksum (mimc.go:130-163): the digest of the integers `elems` from state h"""
    r, cs = curve.r, constants(curve)
    for m in elems:
        t = m
        for c in cs:
            t = pow(t + h + c, 5, r)
        h = (t + h + h + m) % r
    return h


class Hash:
    """the reference's digest over the model: Reset / Write / Sum on big-endian blocks"""

    def __init__(self, curve):
        self.curve, self.bs = curve, 8 * curve.fr_limbs
        self.Reset()

    def Reset(self):
        self.h, self.data = 0, []

    def Write(self, p):
        assert len(p) % self.bs == 0
        self.data += [int.from_bytes(p[i:i + self.bs], "big") for i in range(0, len(p), self.bs)]

    def Sum(self, b=b""):
        self.h, self.data = mimc(self.curve, self.data, self.h), []
        return b + self.h.to_bytes(self.bs, "big")


# ---- the tree. H is a function of byte strings: H(data) a leaf's sum, H(a, b) a node's (the prefixes are commented out).
class StackTree:
    """tree.go restated: Push keeps a stack of complete subtrees [(height, sum)], smallest last, and collects the proof set of
    proof_index on the way; Root and Prove join the smaller subtrees first."""

    def __init__(self, H, proof_index):
        self.H, self.stack, self.current, self.proof_index, self.proof = H, [], 0, proof_index, []

    def Push(self, data):
        if self.current == self.proof_index:
            self.proof.append(data)
        self.stack.append((0, self.H(data)))
        while len(self.stack) >= 2 and self.stack[-1][0] == self.stack[-2][0]:  # joinAllSubTrees
            (h, head), (_, nxt) = self.stack[-1], self.stack[-2]
            if h == len(self.proof) - 1:
                leaves = 1 << h
                mid = self.current // leaves * leaves
                self.proof.append(head if self.proof_index < mid else nxt)
            self.stack[-2:] = [(h + 1, self.H(nxt, head))]
        self.current += 1

    def Root(self):
        if not self.stack:
            return None
        cur = self.stack[-1][1]
        for _, s in reversed(self.stack[:-1]):
            cur = self.H(s, cur)
        return cur

    def Prove(self):
        if not self.stack or not self.proof:
            return self.Root(), None, self.proof_index, self.current
        proof = list(self.proof)
        st = list(self.stack)  # st[-1] is `current`, st[-2] is current.next
        while len(st) >= 2 and st[-2][0] < len(proof) - 1:
            st[-2:] = [(st[-2][0] + 1, self.H(st[-2][1], st[-1][1]))]
        if len(st) >= 2 and st[-2][0] == len(proof) - 1:
            proof.append(st[-1][1])
            st.pop()
        st.pop()  # the subtree that contains the proof index
        while st:
            proof.append(st.pop()[1])
        return self.Root(), proof, self.proof_index, self.current


def stack_tree(H, leaves, index):
    t = StackTree(H, index)
    for d in leaves:
        t.Push(d)
    return t.Prove()


def levels(H, leaves):
    """what the device builds: level 0 = the leaves' sums; each next level pairs the nodes up from the left and moves an odd
    last node up unchanged"""
    out = [[H(d) for d in leaves]]
    while len(out[-1]) > 1:
        lv = out[-1]
        out.append([H(lv[i], lv[i + 1]) if i + 1 < len(lv) else lv[i] for i in range(0, len(lv), 2)])
    return out


def level_proof(lv, leaves, index):
    """(root, proofSet, index, numLeaves) read off the levels: the sibling at every level where the node has one, bottom up"""
    proof, idx = [leaves[index]], index
    for level in lv[:-1]:
        if idx ^ 1 < len(level):
            proof.append(level[idx ^ 1])
        idx >>= 1
    return lv[-1][0], proof, index, len(leaves)


def verify_proof(H, root, proof, index, n):
    """verify.go:31-137"""
    if root is None or index >= n:
        return False
    height = 0
    if len(proof) <= height:
        return False
    acc = H(proof[height])
    height += 1
    stable_end = index
    while True:
        start = index // (1 << height) * (1 << height)
        end = start + (1 << height) - 1
        if end >= n:
            break
        stable_end = end
        if len(proof) <= height:
            return False
        acc = H(acc, proof[height]) if index - start < 1 << (height - 1) else H(proof[height], acc)
        height += 1
    if stable_end != n - 1:
        if len(proof) <= height:
            return False
        acc = H(acc, proof[height])
        height += 1
    while height < len(proof):
        acc = H(proof[height], acc)
        height += 1
    return acc == root


def mimc_H(curve):
    """H over MiMC: the digest of the concatenated big-endian blocks"""
    bs = 8 * curve.fr_limbs

    def H(*data):
        p = b"".join(data)
        return mimc(curve, [int.from_bytes(p[i:i + bs], "big") for i in range(0, len(p), bs)]).to_bytes(bs, "big")
    return H
