"""Launch shapes of the suffix scan (gmsm_poly.h, PolyField::suffix) that the lengths of tests/test_gpu_kzg_open.py do not
select, every output limb for limb against that file's big-int Horner model:
  - the carry pass (the second launch, over the nt tile values) with lanes of 2^tc tiles, tc = 1, 2, 3: a ragged last lane,
    empty lanes, the power index p[b0 + tb + j] at tb > 0. By default that needs more than 2^21 coefficients;
    GMSM_OPT_POLY_LANE_BITS = 1 (lanes of one coefficient, tiles of 256) reaches it at 2^16 + 1
  - every lane width 1 .. 32 on ragged last tiles
  - the default table's switches of the lane width at 2^14 | 2^14 + 1 and 2^18 | 2^18 + 1, unforced
  - the default path at 2^21 + 1 (nt = 257 tiles of 32-coefficient lanes, tc = 1), unforced
  - the callers with other pointer combinations under forced lanes: kzg.Open / BatchOpenSinglePoint (quotient left on the
    device for the MultiExp) and shplonk's chains (value and quotient) and W' (quotient only)"""
import numpy as np
import pytest

import shplonk_model as sm
from conftest import random_field_limbs, rng_for
from test_gpu_kzg_open import CURVES, ints, limbs, model, points_for
from test_gpu_shplonk import check_against_model, mont, rand_true

pytestmark = pytest.mark.gpu

TPB = 256  # lanes per tile (POLY_TPB)
# item 1: lane width 1, tile = 256 coefficients: (length, tiles nt, tc = the smallest with 256 << tc >= nt)
CARRY_LENGTHS = [(256 * 256, 256, 0), (256 * 256 + 1, 257, 1), (256 * 300 + 77, 301, 1), (256 * 512 + 1, 513, 2),
                 (256 * 1024 + 255, 1025, 3), (256 * 777, 777, 2)]
KEY_POINTS = 70000

_POINTS, _POLYS = {}, {}


def _tc(nt):
    tc = 0
    while (TPB << tc) < nt:
        tc += 1
    return tc


def test_the_table_of_carry_lengths_is_what_it_says():
    for n, nt, tc in CARRY_LENGTHS:
        assert (n + TPB - 1) // TPB == nt and _tc(nt) == tc
    assert sorted({tc for _, _, tc in CARRY_LENGTHS}) == [0, 1, 2, 3]
    n = (1 << 21) + 1  # item 4: 32-coefficient lanes
    assert (n + 32 * TPB - 1) // (32 * TPB) == 257 and _tc(257) == 1


def points(gm, curve):
    """0, 1, r - 1 and a random element (limbs, true value), the same four for every test of a curve"""
    if curve not in _POINTS:
        _POINTS[curve] = points_for(gm.CURVES[curve], rng_for(0x5C01, CURVES.index(curve)))
    return _POINTS[curve]


def points_at(gm, curve, n):
    pts = points(gm, curve)
    return pts if n <= (1 << 17) else pts[2:]


def poly(gm, curve, n):
    """(limbs, ints) of the polynomial of length n of a curve, made once"""
    if (curve, n) not in _POLYS:
        c = gm.CURVES[curve]
        f = random_field_limbs(rng_for(0x5C02, CURVES.index(curve), n), c.r, c.fr_limbs, n)
        f.setflags(write=False)
        _POLYS[(curve, n)] = (f, ints(f))
    return _POLYS[(curve, n)]


def check_divide_and_eval(gm, curve, n, pts):
    """DividePolyByXMinusA (quotient and value) and PolyEval (the eval-only form) of the length-n polynomial at pts"""
    c = gm.CURVES[curve]
    f, fi = poly(gm, curve, n)
    for pl, pv in pts:
        mh, mv = model(fi, pv, c.r)
        h, val = gm.kzg.DividePolyByXMinusA(curve, f, pl)
        assert ints(val) == [mv], (n, pv)
        assert h.shape == (n - 1, c.fr_limbs) and ints(h) == mh, (n, pv)
        assert ints(gm.kzg.PolyEval(curve, [f], pl)) == [mv], (n, pv)


@pytest.mark.parametrize("n,nt,tc", CARRY_LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_carry_pass_with_several_tiles_per_lane(gm, forced_options, curve, n, nt, tc):
    forced_options(poly_lane_bits=1)
    check_divide_and_eval(gm, curve, n, points_at(gm, curve, n))


@pytest.mark.parametrize("curve", CURVES)
def test_carry_pass_eval_of_polynomials_at_offsets(gm, forced_options, curve):
    """PolyEval over all the lengths in one list: every polynomial but the first starts at a non-zero offset of the buffer"""
    c = gm.CURVES[curve]
    forced_options(poly_lane_bits=1)
    pl, pv = points(gm, curve)[3]
    polys = [poly(gm, curve, n) for n, _, _ in CARRY_LENGTHS]
    vals = gm.kzg.PolyEval(curve, [f for f, _ in polys], pl)
    assert ints(vals) == [model(fi, pv, c.r)[1] for _, fi in polys]


@pytest.mark.parametrize("curve", CURVES)
def test_carry_pass_tile_power_index_moves_with_the_lane_width(gm, forced_options, curve):
    """lanes of 4: 256 * 512 + 1 is 128 tiles and one coefficient (tc = 0), the tile powers start at p[10] instead of p[8]"""
    forced_options(poly_lane_bits=3)
    n = 256 * 512 + 1
    assert (n + 4 * TPB - 1) // (4 * TPB) == 129
    check_divide_and_eval(gm, curve, n, points_at(gm, curve, n))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("curve", CURVES)
def test_every_lane_width_on_ragged_tiles(gm, forced_options, curve, k):
    forced_options(poly_lane_bits=k)
    T = 1 << (k - 1)
    L = TPB * T
    for n in (L - 1, L, L + 1, 2 * L + T + 1, 3 * L - 1):
        check_divide_and_eval(gm, curve, n, points_at(gm, curve, n))


@pytest.mark.parametrize("n", [1 << 14, (1 << 14) + 1, 1 << 18, (1 << 18) + 1, (1 << 18) + 8192 + 5])
@pytest.mark.parametrize("curve", ["bn254", "bw6_761"])
def test_default_table_switches(gm, curve, n):
    """lanes of 8 up to 2^14, 16 up to 2^18, 32 above; 2^18 + 8192 + 5: a ragged last tile of 32-coefficient lanes"""
    assert gm.get_option("poly_lane_bits") == 0
    check_divide_and_eval(gm, curve, n, points_at(gm, curve, n))


def test_default_path_above_2_pow_21(gm):
    """BN254, 2^21 + 1 coefficients, nothing forced: 257 tiles of 32-coefficient lanes, the carry pass with two tiles per
    lane. The division at the random point and the eval-only form at r - 1. Its time is the Python model's."""
    curve = "bn254"
    c = gm.CURVES[curve]
    assert gm.get_option("poly_lane_bits") == 0
    n = (1 << 21) + 1
    f, fi = poly(gm, curve, n)
    pts = points(gm, curve)
    pl, pv = pts[3]
    mh, mv = model(fi, pv, c.r)
    h, val = gm.kzg.DividePolyByXMinusA(curve, f, pl)
    assert ints(val) == [mv]
    assert h.shape == (n - 1, c.fr_limbs) and ints(h) == mh
    del mh, h
    pl, pv = pts[2]
    assert ints(gm.kzg.PolyEval(curve, [f], pl)) == [model(fi, pv, c.r)[1]]
    del _POLYS[(curve, n)]


@pytest.fixture(scope="module")
def keys(gm):
    """registered keys of KEY_POINTS points made on the device (BatchScalarMultiplication of a fixed point), one per curve"""
    made = {}

    def get(curve):
        if curve not in made:
            c = gm.CURVES[curve]
            g = gm.G1Affine(curve)
            gen = np.array(g.generate_points(1, 0xC0FFEE, 0xBEEF)[0], dtype=np.uint64)
            sc = random_field_limbs(rng_for(0x5C03, CURVES.index(curve)), c.r, c.fr_limbs, KEY_POINTS)
            made[curve] = (g, g.register_bases(points=g.BatchScalarMultiplication(gen, sc)))
        return made[curve]
    yield get
    for _, rb in made.values():
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_open_commits_the_model_quotient_forced_lanes(gm, forced_options, keys, curve):
    c = gm.CURVES[curve]
    g, rb = keys(curve)
    forced_options(poly_lane_bits=1)
    n = 256 * 256 + 1
    f, fi = poly(gm, curve, n)
    pl, pv = points(gm, curve)[3]
    claimed, H = gm.kzg.Open(f, pl, rb)
    mh, mv = model(fi, pv, c.r)
    jac, err = rb.MultiExp(limbs(mh, c.fr_limbs))
    assert err is None
    assert ints(claimed) == [mv]
    assert (H == g.jac_to_affine(jac)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_batch_open_matches_fold_then_divide_forced_lanes(gm, forced_options, keys, curve):
    c = gm.CURVES[curve]
    g, rb = keys(curve)
    forced_options(poly_lane_bits=1)
    pts = points(gm, curve)
    pl, pv = pts[3]
    gl, gv = pts[2]  # gamma = r - 1
    lens = (1, 65537, 300)
    polys = [poly(gm, curve, n) for n in lens]
    values, H = gm.kzg.BatchOpenSinglePoint([f for f, _ in polys], pl, gl, rb)
    assert ints(values) == [model(fi, pv, c.r)[1] for _, fi in polys]
    maxlen = max(lens)
    F = [0] * maxlen
    for _, pi in reversed(polys):  # sum_i gamma^i f_i (Horner in gamma, on Montgomery representatives: gamma's true value)
        F = [(F[j] * gv + (pi[j] if j < len(pi) else 0)) % c.r for j in range(maxlen)]
    mh, _ = model(F, pv, c.r)
    jac, err = rb.MultiExp(limbs(mh, c.fr_limbs))
    assert err is None and (H == g.jac_to_affine(jac)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_shplonk_forced_lanes(gm, forced_options, keys, curve):
    """OpenW's chains (lengths 65540 and 65539: 257 tiles, quotient and remainder) and OpenWPrime's division (quotient only)
    with two tiles per lane of the carry pass, against the reference-as-written model"""
    c = gm.CURVES[curve]
    g, rb = keys(curve)
    lens, sizes = (65537 + 3, 100), (2, 1)
    assert KEY_POINTS >= max(lens) + sum(sizes) - 1
    rng = rng_for(0x5C04, CURVES.index(curve))
    pa, pb, pc = rand_true(c, rng, 3)
    pts = [[pa, pb], [pc]]
    polys = [rand_true(c, rng, n) for n in lens]
    gamma, z = rand_true(c, rng, 2)
    w, claimed, wprime = sm.reference_batch_open(polys, pts, gamma, z, c.r)
    case = dict(polys=[mont(c, p) for p in polys], points=[mont(c, s) for s in pts], gamma=mont(c, [gamma])[0], z=mont(c, [z])[0],
                w=w, claimed=claimed, wprime=wprime)
    forced_options(poly_lane_bits=1)
    check_against_model(gm, c, g, rb, case)
