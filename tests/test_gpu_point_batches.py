"""The point-batch kernels past the sizes the older suites stop at (tests/point_batch_cases.py builds the inputs,
tests/test_point_batch_cases.py shows on the host that each has the property it is named for), limb for limb:
  - k_fixed_base at the table widths GMSM_OPT_FIXED_BASE_BITS admits: windows that straddle the scalar's 32-bit words in every
    way, the widths that divide the scalar size (a doubled top bucket set), scalars whose every window borrows - each result
    against the oracle's own double-and-add; BW6-761 G2 included
  - k_batch_normalize with whole K-record groups at infinity (the inversion of an untouched one), an infinity first and last in a
    group, n on either side of a group and of a workgroup, through BatchJacobianToAffine and BatchScalarMultiplication
  - the GLV walk over one table entry only, and with every sign mix the split returns, per point and one scalar for all
  - Group::batch_scale beyond one chunk of 2^18 lanes: the second launch's record and table indices, the reuse of the table,
    the upper bits of the powers ladder, infinities and special scalars on both sides of the seam"""
import numpy as np
import pytest

import frontend_cases as fc
import point_batch_cases as pc
from conftest import ALL_GROUPS, rng_for
from test_gpu_mpcsetup import case_of, group_of, mirror, points_of, random_ints, special_scalars

pytestmark = pytest.mark.gpu

IDS = [f"{c}-{w}" for c, w in ALL_GROUPS]
MASK64 = (1 << 64) - 1


def is_wide(curve, which):
    return which == "g2" or curve == "bw6_761"


def patterns_of(gm, curve):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the dropped pairs are reported by tests/test_point_batch_cases.py
        return pc.glv_pattern_cases(curve)


def points_fast(gm, curve, which, vals):
    """points_of() for the large batches: [v]Gen through the fixed-base batch"""
    g = group_of(gm, curve, which)
    return g.BatchScalarMultiplication(g.generator, fc.mont_limbs(gm.CURVES[curve], vals))


def first_mismatches(got, exp):
    return [int(i) for i in np.nonzero((got != exp).any(axis=1))[0][:8]]


# ------------------------------------------------------------------ fixed base: widths and borrow chains
_bases = {}


def other_base(o):
    """a base that is not the generator"""
    if o.name not in _bases:
        _bases[o.name] = o.gen_points(8, 0xB45E + (o.curve.r >> 5), 0x9E3779B97F4A7C15, nthreads=4)[7]
    return _bases[o.name]


@pytest.mark.parametrize("curve,which,c", pc.FIXED_BASE_CASES, ids=[f"{cu}-{w}-{c}" for cu, w, c in pc.FIXED_BASE_CASES])
def test_fixed_base_widths_and_borrow_chains(gm, oracle_mod, forced_options, curve, which, c):
    forced_options(fixed_base_bits=c)
    g, o, cv = group_of(gm, curve, which), oracle_mod.Oracle(curve, which), gm.CURVES[curve]
    base = other_base(o)
    cases = pc.borrow_cases(cv, c)
    names = [name for name, _, _ in cases] + ["random"] * 16
    vals = [s for _, s, _ in cases] + random_ints(rng_for(0x9B0, ALL_GROUPS.index((curve, which)), c), cv, 16)
    got = g.BatchScalarMultiplication(base, fc.mont_limbs(cv, vals))
    for i, k in enumerate(vals):
        exp = o.jac_to_affine(o.scalar_mul(base, k)) if k else np.zeros(g.aff_limbs, dtype=np.uint64)
        assert (got[i] == exp).all(), (curve, which, c, names[i], hex(k))


# ------------------------------------------------------------------ normalisation: whole groups at infinity
def _elems(row, fl):
    return [int.from_bytes(row[i:i + fl].tobytes(), "little") for i in range(0, len(row), fl)]


def _mul(a, b, p):
    """in Fp (one component) or Fp2 = Fp[u] / (u^2 + 1)"""
    if len(a) == 1:
        return [a[0] * b[0] % p]
    return [(a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p]


def jacobian_of(cv, ext, aff, rng):
    """(x lam^2, y lam^3, lam) with a random lam of the coordinate field for every affine (x, y): Python integers on the
    Montgomery limbs (v R mod p as stored; a product of two stored values is brought back by R^-1)"""
    p, fl = cv.p, cv.fp_limbs
    cl = fl * ext
    rinv = pow(cv.fp_R, -1, p)
    out = np.zeros((len(aff), 3 * cl), dtype=np.uint64)
    for i, row in enumerate(aff):
        x, y = _elems(row[:cl], fl), _elems(row[cl:], fl)
        lam = [int.from_bytes(rng.bytes(8 * fl), "little") % p for _ in range(ext)]  # lam R: uniform, like lam
        lam[0] = lam[0] or 1
        mm = lambda a, b: [v * rinv % p for v in _mul(a, b, p)]  # the Montgomery product of stored values
        l2 = mm(lam, lam)
        coords = mm(x, l2) + mm(y, mm(l2, lam)) + lam
        out[i] = [(v >> (64 * k)) & MASK64 for v in coords for k in range(fl)]
    return out


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_whole_groups_at_infinity(gm, oracle_mod, curve, which):
    g, o, cv = group_of(gm, curve, which), oracle_mod.Oracle(curve, which), gm.CURVES[curve]
    sizes = pc.NORMALIZE_SIZES_WIDE if is_wide(curve, which) else pc.NORMALIZE_SIZES
    nmax, cl = max(sizes), g.coord_limbs
    rng = rng_for(0x9B1, ALL_GROUPS.index((curve, which)))
    k0, k1 = 0x5EED + (cv.r >> 7), 0xC2B2AE3D27D4EB4F
    aff = o.gen_points(nmax, k0, k1, nthreads=8)
    assert aff.any(axis=1).all()
    jac = jacobian_of(cv, o.ext, aff, rng)
    assert (g.BatchJacobianToAffine(jac[:65]) == aff[:65]).all(), "no infinity at all"
    garbage = rng.integers(0, 2**64, size=(nmax, 2 * cl), dtype=np.uint64)
    sc = fc.mont_limbs(cv, [(k0 + i * k1) % cv.r for i in range(nmax)])
    for n in sizes:
        for name, mask in pc.infinity_masks(n):
            m = np.array(mask, dtype=bool)
            exp = aff[:n].copy()
            exp[m] = 0
            j = jac[:n].copy()
            j[m, 2 * cl:] = 0                 # Z = 0 ...
            j[m, :2 * cl] = garbage[:n][m]    # ... and whatever in X and Y
            got = g.BatchJacobianToAffine(j)
            assert (got == exp).all(), (curve, which, "BatchJacobianToAffine", n, name, first_mismatches(got, exp))
            s = sc[:n].copy()
            s[m] = 0                          # the scalar 0: a record at infinity out of k_fixed_base
            got = g.BatchScalarMultiplication(o.generator, s)
            assert (got == exp).all(), (curve, which, "BatchScalarMultiplication", n, name, first_mismatches(got, exp))


# ------------------------------------------------------------------ the walk: table selection
@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_walk_over_one_table_entry(gm, oracle_mod, curve, which):
    cv, o = gm.CURVES[curve], oracle_mod.Oracle(curve, which)
    pats = patterns_of(gm, curve)
    rng = rng_for(0x9B2, ALL_GROUPS.index((curve, which)))
    # per point: every pattern scalar on three finite points and on one at infinity
    ks = random_ints(rng, cv, 3) + [0]
    k = [a for a in ks for _ in pats]
    s = [p[3] for _ in ks for p in pats]
    pts = points_of(gm, curve, which, k)
    assert not pts[-1].any() and pts[0].any()
    got = mirror(gm, which, "BatchScale")(curve, pts, fc.mont_limbs(cv, s))
    exp = points_of(gm, curve, which, [a * b % cv.r for a, b in zip(k, s)])
    bad = first_mismatches(got, exp)
    assert not bad, (curve, which, [(pats[i % len(pats)][0], hex(k[i])) for i in bad])
    # ... 8 of them against the oracle's double-and-add: the expectation does not rest on the fixed-base kernel alone
    for i in range(8):
        assert (got[i] == o.jac_to_affine(o.scalar_mul(pts[i], s[i]))).all(), (curve, which, pats[i % len(pats)][0])
    # one scalar for all: the whole wave takes one table entry together
    kk, _, base_pts, _ = case_of(gm, curve, which)
    n = 65
    assert len(kk) >= n
    for name, _, _, sv in pats:
        got = mirror(gm, which, "Scale")(curve, base_pts[:n], fc.mont_limbs(cv, [sv]))
        exp = points_of(gm, curve, which, [a * sv % cv.r for a in kk[:n]])
        assert (got == exp).all(), (curve, which, name, first_mismatches(got, exp))


# ------------------------------------------------------------------ batch_scale: the second chunk
SEAM = pc.SCALE_CHUNK
N_TWO_CHUNKS = SEAM + 257
_two_chunks = {}


def seam_report(got, exp):
    bad = first_mismatches(got, exp)
    return [(i, "first chunk" if i < SEAM else "second chunk, lane %d" % (i - SEAM)) for i in bad]


def two_chunk_case(gm, curve, which):
    """k (every 7th 0, from index 4: the records 2^18 - 3 .. 2^18 + 2 on both sides of the seam are finite as made), s (the special
    and the pattern scalars in one block across the seam; the block is longer than 7, so two of its scalars, at 2^18 - 4 and
    2^18 + 3, meet an infinity in both variants), A = [k]Gen for n = 2^18 + 257 - made once"""
    key = (curve, which)
    if key not in _two_chunks:
        cv = gm.CURVES[curve]
        n = N_TWO_CHUNKS
        rng = rng_for(0x9B3, ALL_GROUPS.index(key))
        k, s = random_ints(rng, cv, n), random_ints(rng, cv, n)
        for i in range(4, n, 7):
            k[i] = 0
        assert all(k[i] for i in range(SEAM - 3, SEAM + 3)) and k[n - 1] and not k[SEAM - 4] and not k[SEAM + 3]
        sp = special_scalars(gm, cv) + [p[3] for p in patterns_of(gm, curve)]
        assert len(sp) >= 5
        first = SEAM - len(sp) // 2
        assert first <= SEAM - 2 and first + len(sp) - 1 >= SEAM + 2
        s[first:first + len(sp)] = sp
        pts = points_fast(gm, curve, which, k)
        pts.setflags(write=False)
        _two_chunks[key] = (k, s, pts)
    return _two_chunks[key]


def seam_variants(k, pts):
    """the case as made, and with k = 0 forced on both sides of the seam and at the end"""
    yield "as made", k, pts
    k2, p2 = list(k), pts.copy()
    for i in (SEAM - 1, SEAM, len(k) - 1):
        k2[i] = 0
        p2[i] = 0
    yield "infinity at the seam", k2, p2


@pytest.mark.parametrize("form", ["per_point", "one_scalar", "powers"])
def test_second_chunk_bn254_g1(gm, form):
    curve, which = "bn254", "g1"
    cv = gm.CURVES[curve]
    k, s, pts = two_chunk_case(gm, curve, which)
    n = len(k)
    assert n > pc.SCALE_CHUNK and n - pc.SCALE_CHUNK == 257
    rng = rng_for(0x9B4)
    one = random_ints(rng, cv, 2)
    if form == "per_point":
        mult, args = s, fc.mont_limbs(cv, s)
        run = lambda a: mirror(gm, which, "BatchScale")(curve, a, args)
    elif form == "one_scalar":
        mult, args = [one[0]] * n, fc.mont_limbs(cv, one[:1])
        run = lambda a: mirror(gm, which, "Scale")(curve, a, args)
    else:
        mult, acc = [], 1
        for _ in range(n):  # r^i: bits 18 and up of i in the second chunk
            mult.append(acc)
            acc = acc * one[1] % cv.r
        args = fc.mont_limbs(cv, one[1:])
        run = lambda a: mirror(gm, which, "UpdateMonomials")(curve, a, args)
    exp = points_fast(gm, curve, which, [a * b % cv.r for a, b in zip(k, mult)])
    for name, kv, a in seam_variants(k, pts):
        e = exp
        if kv is not k:
            e = exp.copy()
            e[[i for i in range(n) if kv[i] == 0]] = 0
        keep = a.copy()
        got = run(a)
        assert (a == keep).all()
        assert (got == e).all(), (form, name, seam_report(got, e))
        assert not got[SEAM - 4].any() and (kv is k or not (got[SEAM - 1].any() or got[SEAM].any() or got[n - 1].any()))
    assert exp[SEAM - 1].any() and exp[SEAM].any() and exp[n - 1].any()  # finite on both sides of the seam as made


def test_second_chunk_in_place_then_a_small_batch(gm):
    """the device-pointer entry with the output on the input, and straight after it a 1000-point call on the same thread: the
    walk's table has just been sized and filled by the large call"""
    import torch
    curve, which = "bn254", "g1"
    cv = gm.CURVES[curve]
    k, s, pts = two_chunk_case(gm, curve, which)
    n = len(k)
    exp = points_fast(gm, curve, which, [a * b % cv.r for a, b in zip(k, s)])
    d = torch.from_numpy(pts.view(np.int64).copy()).cuda()
    dsc = torch.from_numpy(fc.mont_limbs(cv, s).view(np.int64)).cuda()
    torch.cuda.synchronize()
    gm.mpcsetup.batch_scale_device(curve, which, d.data_ptr(), n, dsc.data_ptr(), n, d.data_ptr(), 0)
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint64).reshape(pts.shape)
    assert (got == exp).all(), seam_report(got, exp)
    ks, ss, small, small_exp = case_of(gm, curve, which)
    assert len(ks) == 1000
    got = mirror(gm, which, "BatchScale")(curve, small, fc.mont_limbs(cv, ss))
    assert (got == small_exp).all(), first_mismatches(got, small_exp)


def test_second_chunk_bls12_381_g2(gm):
    """the largest record (448 bytes) and 3 x 2^18 table slots of it; the per-point form only"""
    curve, which = "bls12_381", "g2"
    cv = gm.CURVES[curve]
    k, s, pts = two_chunk_case(gm, curve, which)
    exp = points_fast(gm, curve, which, [a * b % cv.r for a, b in zip(k, s)])
    sc = fc.mont_limbs(cv, s)
    for name, kv, a in seam_variants(k, pts):
        e = exp
        if kv is not k:
            e = exp.copy()
            e[[i for i in range(len(k)) if kv[i] == 0]] = 0
        got = mirror(gm, which, "BatchScale")(curve, a, sc)
        assert (got == e).all(), (name, seam_report(got, e))
