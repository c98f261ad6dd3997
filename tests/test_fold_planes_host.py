"""GroupHost::fold_planes through gmsm_debug_fold_planes, no device: planes [k]G with known k (extended coordinates with a
random zz, so that no addition is a mixed one) against the big-integer model,
    sum_w 2^(c w) (k_w0 + sum_(i>=1) 2^(log2L + i - 1) k_wi)  [G],
affine limb for limb. Shapes: the headline's (c = 16, L = 8, 128 blocks: 14 planes per window), one block (7 planes), a width
below the span of a window's planes (neighbouring windows share bit positions), nwin = 1; planes at infinity, a window
whose planes are all infinite, an all-infinite input, and sums that meet P + P and P - P inside the walk."""
import ctypes
import random

import numpy as np
import pytest

from conftest import ALL_GROUPS


def one_limbs(curve, ext):
    import pyref
    return pyref.fp_to_mont(curve, 1) + ([0] * curve.fp_limbs if ext == 2 else [])


def plane_limbs(pg, rng, k):
    """[k]G as x, y, zz, zzz with zz = lam^2 for a random lam (k = 0 or None: infinity, (1, 1, 0, 0))"""
    import pyref
    n, ext = pg.c.fp_limbs, pg.ext
    P = pg.mul(k, pg.gen) if k else None
    if P is None:
        return one_limbs(pg.c, ext) * 2 + [0] * (2 * n * ext)
    lam = rng.randrange(2, pg.p)
    l2, l3 = lam * lam % pg.p, lam * lam * lam % pg.p
    x, y = P
    if ext == 1:
        vals = [x * l2 % pg.p, y * l3 % pg.p, l2, l3]
        return [v for c in vals for v in pyref.fp_to_mont(pg.c, c)]
    vals = [(x.a0 * l2 % pg.p, x.a1 * l2 % pg.p), (y.a0 * l3 % pg.p, y.a1 * l3 % pg.p), (l2, 0), (l3, 0)]
    return [v for a0, a1 in vals for v in pyref.fp_to_mont(pg.c, a0) + pyref.fp_to_mont(pg.c, a1)]


def expected(pg, ks, c, log2L):
    r = pg.c.r
    tot = 0
    for w, row in enumerate(ks):
        tot += sum((k or 0) << (0 if i == 0 else log2L + i - 1) for i, k in enumerate(row)) << (c * w)
    return np.array(pg.point_to_limbs(pg.mul(tot % r, pg.gen) if tot % r else None), dtype=np.uint64)


def run(g, pg, rng, ks, c, log2L, nblocks1):
    nwin = len(ks)
    assert all(len(row) == 7 + (nblocks1 - 1).bit_length() for row in ks)
    planes = np.array([plane_limbs(pg, rng, k) for row in ks for k in row], dtype=np.uint64)
    jac = g.fold_planes(planes, c, nwin, log2L, nblocks1)
    want = expected(pg, ks, c, log2L)
    if not want.any():
        assert not jac[2 * g.coord_limbs:].any(), "expected infinity (z = 0)"
    assert (g.jac_to_affine(jac) == want).all()
    return jac


SHAPES = [(16, 8, 3, 128), (11, 3, 4, 1), (7, 4, 3, 40), (13, 1, 1, 2)]  # (c, nwin, log2L, nblocks1)


@pytest.mark.parametrize("c,nwin,log2L,nblocks1", SHAPES)
@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_fold_planes_matches_the_model(gm, pyref_mod, curve, which, c, nwin, log2L, nblocks1):
    g = (gm.G1Jac if which == "g1" else gm.G2Jac)(curve)
    pg = pyref_mod.Group(g.curve, which)
    rng = random.Random(f"fold_planes/{curve}/{which}/{c}/{nwin}")
    NP = 7 + (nblocks1 - 1).bit_length()
    r = g.curve.r
    dense = [[rng.randrange(1, r) for _ in range(NP)] for _ in range(nwin)]
    run(g, pg, rng, dense, c, log2L, nblocks1)
    # planes at infinity here and there, the top plane of the top window among them; one window without a finite plane
    holes = [[None if rng.randrange(3) == 0 else k for k in row] for row in dense]
    holes[-1][-1] = None
    holes[nwin // 2] = [None] * NP
    run(g, pg, rng, holes, c, log2L, nblocks1)
    # nothing but one plane
    single = [[None] * NP for _ in range(nwin)]
    single[0][1] = 7
    run(g, pg, rng, single, c, log2L, nblocks1)


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_all_infinite_is_infinity(gm, pyref_mod, curve, which):
    g = (gm.G1Jac if which == "g1" else gm.G2Jac)(curve)
    pg = pyref_mod.Group(g.curve, which)
    rng = random.Random("fold_planes/inf")
    for c, nwin, log2L, nblocks1 in SHAPES:
        NP = 7 + (nblocks1 - 1).bit_length()
        jac = run(g, pg, rng, [[None] * NP for _ in range(nwin)], c, log2L, nblocks1)
        assert not jac[2 * g.coord_limbs:].any()


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bn254", "g2"), ("bw6_761", "g1")])
def test_doubling_and_cancelling_inside_the_walk(gm, pyref_mod, curve, which):
    """one window, L = 2, one block: plane i sits at bit i. k_5 = 2 k_6 makes the addition at bit 5 a P + P, k_4 = -8 k_6 the one
    at bit 4 a P - P (the walk goes on from infinity), and the planes below build a finite sum again"""
    g = (gm.G1Jac if which == "g1" else gm.G2Jac)(curve)
    pg = pyref_mod.Group(g.curve, which)
    rng = random.Random(f"fold_planes/collide/{curve}/{which}")
    r = g.curve.r
    k6 = rng.randrange(1, r)
    ks = [[rng.randrange(1, r), rng.randrange(1, r), None, rng.randrange(1, r), (-8 * k6) % r, 2 * k6 % r, k6]]
    run(g, pg, rng, ks, 16, 1, 1)
    ks[0][3] = None  # ... and with nothing at bit 3: the sum stays infinite over a run of doublings
    run(g, pg, rng, ks, 16, 1, 1)


def test_arguments_are_checked(gm):
    lib = gm._lib.load()
    g = gm.G1Jac("bn254")
    buf = np.zeros(13 * 8 * g.xyzz_limbs, dtype=np.uint64)
    out = np.zeros(g.jac_limbs, dtype=np.uint64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = [(99, 16, 8, 3, 64), (g.gid, 1, 8, 3, 64), (g.gid, 16, 0, 3, 64), (g.gid, 16, 8, 9, 64), (g.gid, 16, 8, 3, 0), (g.gid, 16, 8, 3, 129)]
    for gid, c, nwin, log2L, nb in bad:
        assert lib.gmsm_debug_fold_planes(gid, c, nwin, log2L, nb, P(buf), P(out)) == gm._lib.GMSM_ERR_ARG
    assert lib.gmsm_debug_fold_planes(g.gid, 16, 8, 3, 64, None, P(out)) == gm._lib.GMSM_ERR_ARG
