"""The field products of the lazy-limb code (gmsm_fieldu.h: chained product scans, the two-at-once forms the mixed addition
runs) on the device, through the debug hooks, against a Python big-integer model - all six groups, vectors of 1 to 64
elements, limbs compared for equality.

Products and squares (gmsm_debug_field_op, field 3 = the coordinate field through the lazy code): the words 0, 1, q - 1, q,
2q - 1 and 2^(64 n) - 1 (every limb of the unpacked operand at its largest) in all pairs, and random elements.

Mixed additions (gmsm_debug_group_op, ops 4 and 5 = the accumulation loop's addition and subtraction): accumulator at
infinity, P + P with ZZ = 1 and with ZZ != 1, P + (-P), a base with x = 0, ordinary additions - and the false positives of
the cheap P == 0 test: accumulators built so that the FIRST LIMB of PP = P^2, as the product scan returns it, equals the
first limb of 0, of q or of 2q while PP is not zero. The scan returns the integer V = (P'^2 + M q) / R' with R' = 2^(L W),
the unique member of [P'^2 / R', P'^2 / R' + q) in the residue class of P^2 R' (P' = the integer the device holds for P);
with |P'| below 8q that interval starts below q / 2, so for a chosen V in (q / 2, q) with the wanted low limb any P with
P^2 = V / R' mod q makes the device compute exactly that V. A draw at random hits the path once in 2^28."""
import ctypes

import numpy as np
import pytest

from conftest import ALL_GROUPS, int_to_limbs, rng_for

pytestmark = pytest.mark.gpu

PTR = lambda a: a.ctypes.data_as(ctypes.c_void_p)
LAZY = {"bn254": (9, 29), "bls12_381": (14, 28), "bw6_761": (28, 28)}  # limbs x bits of the base fields (gmsm_params32.h)


class F:
    """An element of Fp (ext 1) or Fp2 = Fp[u]/(u^2 + 1) (ext 2) as Python integers."""

    def __init__(self, p, a0, a1=0):
        self.p, self.a0, self.a1 = p, a0 % p, a1 % p

    def __add__(self, o): return F(self.p, self.a0 + o.a0, self.a1 + o.a1)
    def __sub__(self, o): return F(self.p, self.a0 - o.a0, self.a1 - o.a1)
    def __neg__(self): return F(self.p, -self.a0, -self.a1)
    def __mul__(self, o):
        if isinstance(o, int):
            return F(self.p, self.a0 * o, self.a1 * o)
        return F(self.p, self.a0 * o.a0 - self.a1 * o.a1, self.a0 * o.a1 + self.a1 * o.a0)
    def is_zero(self): return self.a0 == 0 and self.a1 == 0


def madd(acc, pt, neg):
    """madd-2008-s on XYZZ coordinates with every special case; acc = None is infinity."""
    x, y = pt
    if neg:
        y = -y
    one = F(x.p, 1)
    if acc is None:
        return (x, y, one, one)
    X, Y, ZZ, ZZZ = acc
    Pv, Rv = x * ZZ - X, y * ZZZ - Y
    if Pv.is_zero():
        if not Rv.is_zero():
            return None
        U = y * 2
        V = U * U
        W = U * V
        S = x * V
        M = x * x * 3
        X3 = M * M - S * 2
        return (X3, M * (S - X3) - W * y, V, W)
    PP = Pv * Pv
    PPP = Pv * PP
    Q = X * PP
    X3 = Rv * Rv - PPP - Q * 2
    return (X3, Rv * (Q - X3) - Y * PPP, ZZ * PP, ZZZ * PPP)


def _words(c, ext, v):  # Montgomery limbs of a coordinate
    R = c.fp_R
    out = int_to_limbs(v.a0 * R % c.p, c.fp_limbs)
    if ext == 2:
        out += int_to_limbs(v.a1 * R % c.p, c.fp_limbs)
    return out


def _xyzz_words(c, ext, acc):
    if acc is None:
        return [0] * (4 * ext * c.fp_limbs)
    return sum((_words(c, ext, v) for v in acc), [])


def _false_positive_P(c, target_limb, rng):
    """P in Fp with P^2 R' = V mod q for some V in (q/2, q) whose first limb is target_limb."""
    L, W = LAZY[c.name]
    p = c.p
    assert p % 4 == 3
    Rl = 1 << (L * W)
    while True:
        V = (int(rng.integers(0, 1 << 62)) << (p.bit_length() - 63)) % p
        V = (V >> W << W) | target_limb
        if not p // 2 < V < p:
            continue
        sq = V * pow(Rl, -1, p) % p
        s = pow(sq, (p + 1) // 4, p)
        if s * s % p == sq:
            assert V % (1 << W) == target_limb and V % p != 0
            return s


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_lazy_products_and_squares_on_edge_words(gm, curve, which):
    L = gm._lib.load()
    g = (gm.G1Affine if which == "g1" else gm.G2Affine)(curve)
    c = g.curve
    nl, p, R = c.fp_limbs, c.p, c.fp_R
    ext = g.coord_limbs // nl
    rng = rng_for(0x9c1, g.gid)
    edges = [0, 1, p - 1, p, 2 * p - 1, (1 << (64 * nl)) - 1]
    rnd = lambda: int.from_bytes(rng.bytes(8 * nl + 8), "little") % p
    if ext == 1:
        pairs = [((x,), (y,)) for x in edges for y in edges]
    else:  # every edge in either component, against every edge
        pairs = [((x, y), (y, x)) for x in edges for y in edges]
    pairs += [(tuple(rnd() for _ in range(ext)), tuple(rnd() for _ in range(ext))) for _ in range(64 - len(pairs))]
    assert len(pairs) == 64
    a = np.array([sum((int_to_limbs(v, nl) for v in x), []) for x, _ in pairs], dtype=np.uint64)
    b = np.array([sum((int_to_limbs(v, nl) for v in y), []) for _, y in pairs], dtype=np.uint64)
    Ri = pow(R, -1, p)

    def mul(x, y):  # on the stored words: Montgomery product x y / R
        if ext == 1:
            return int_to_limbs(x[0] * y[0] * Ri % p, nl)
        return int_to_limbs((x[0] * y[0] - x[1] * y[1]) * Ri % p, nl) + int_to_limbs((x[0] * y[1] + x[1] * y[0]) * Ri % p, nl)

    exp_mul = np.array([mul(x, y) for x, y in pairs], dtype=np.uint64)
    exp_sqr = np.array([mul(x, x) for x, _ in pairs], dtype=np.uint64)
    for count in (64, 1, 37):  # more than one wave's worth is not needed: one element per lane, no shared state
        out = np.zeros((count, g.coord_limbs), dtype=np.uint64)
        assert L.gmsm_debug_field_op(g.gid, 3, 0, PTR(a[-count:].copy()), PTR(b[-count:].copy()), count, PTR(out)) == 0, gm._lib.last_error()
        assert (out == exp_mul[-count:]).all(), ("product", count, np.nonzero((out != exp_mul[-count:]).any(axis=1))[0])
        out = np.zeros((count, g.coord_limbs), dtype=np.uint64)
        assert L.gmsm_debug_field_op(g.gid, 3, 5, PTR(a[:count].copy()), None, count, PTR(out)) == 0, gm._lib.last_error()
        assert (out == exp_sqr[:count]).all(), ("square", count, np.nonzero((out != exp_sqr[:count]).any(axis=1))[0])


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_mixed_addition_special_cases_and_zero_test_false_positives(gm, curve, which):
    L = gm._lib.load()
    g = (gm.G1Affine if which == "g1" else gm.G2Affine)(curve)
    c = g.curve
    nl, p = c.fp_limbs, c.p
    ext = g.coord_limbs // nl
    W = LAZY[c.name][1]
    rng = rng_for(0x9c2, g.gid)
    rnd = lambda: F(p, *(int.from_bytes(rng.bytes(8 * nl + 8), "little") for _ in range(ext)))
    scaled = lambda x, y, lam: (x * (lam * lam), y * (lam * lam * lam), lam * lam, lam * lam * lam)  # the point (x, y) with ZZ = lam^2
    one = F(p, 1)
    cases = []  # (accumulator or None, (x, y)): the formulas are identities, so any field elements serve as coordinates
    x, y = rnd(), rnd()
    cases.append((None, (x, y)))                                        # accumulator at infinity
    cases.append(((x, y, one, one), (x, y)))                            # P + P, ZZ = 1
    x, y = rnd(), rnd()
    cases.append((scaled(x, y, rnd()), (x, y)))                         # P + P, ZZ != 1
    x, y = rnd(), rnd()
    cases.append(((x, -y, one, one), (x, y)))                           # P + (-P)
    x, y = rnd(), rnd()
    cases.append((scaled(x, -y, rnd()), (x, y)))                        # P + (-P), ZZ != 1
    cases.append((scaled(rnd(), rnd(), rnd()), (F(p, 0), rnd())))       # a base with x = 0
    cases.append(((F(p, 0), rnd(), one, one), (F(p, 0), rnd())))        # ... onto an accumulator with x = 0: same x
    # the first limb of PP at the first limb of 0, q, 2q, PP itself not zero: accumulator (X, Y, 1, 1), base (X + P, y)
    n_fp = 0
    for target in (0, p % (1 << W), 2 * p % (1 << W)):
        for _ in range(2):
            Pv = F(p, _false_positive_P(c, target, rng))
            X = rnd()
            cases.append(((X, rnd(), one, one), (X + Pv, rnd())))
            n_fp += 1
    while len(cases) < 64:                                              # ordinary additions
        cases.append((scaled(rnd(), rnd(), rnd()), (rnd(), rnd())))
    accs = np.array([_xyzz_words(c, ext, a) for a, _ in cases], dtype=np.uint64)
    pts = np.array([_words(c, ext, pt[0]) + _words(c, ext, pt[1]) for _, pt in cases], dtype=np.uint64)
    cl = g.coord_limbs
    for op, neg in ((4, False), (5, True)):
        # for the subtraction the base goes in negated, so that every case keeps its meaning
        use = pts.copy()
        if neg:
            use = np.array([_words(c, ext, pt[0]) + _words(c, ext, -pt[1]) for _, pt in cases], dtype=np.uint64)
        exp = [madd(a, pt, False) for a, pt in cases]
        assert exp[3] is None and exp[4] is None and exp[6] is None  # same x, another y: the formulas answer infinity
        for count in (64, 1, 13 + n_fp):
            out = np.zeros((count, 4 * cl), dtype=np.uint64)
            assert L.gmsm_debug_group_op(g.gid, op, PTR(accs[:count].copy()), PTR(use[:count].copy()), count, PTR(out)) == 0, gm._lib.last_error()
            for i in range(count):
                if exp[i] is None:
                    assert (out[i, 2 * cl:] == 0).all(), ("infinity expected", op, i)
                else:
                    assert (out[i] == np.array(_xyzz_words(c, ext, exp[i]), dtype=np.uint64)).all(), ("mixed addition", op, i)
