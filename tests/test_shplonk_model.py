"""The shortcut of gmsm_shplonk.h is the reference's function (no GPU, no library): tests/shplonk_model.py restates
shplonk.BatchOpen as written (buildZtMinusSi, interpolate, the naive mul and div, L padded to totalSize) and the chain /
Newton-form / accumulate formulation the device runs; the two must agree on w (trailing zeros stripped), on the claimed
values and on w', over the three scalar fields, for every pair of lengths in 1..12 and set sizes in 1..3 - which covers
polynomials shorter than or as long as their set (empty quotient, r_i = f_i) - with and without a point shared between the
two sets, and for three polynomials."""
import itertools

import pytest

import shplonk_model as sm
from conftest import rng_for

CURVES = ["bn254", "bls12_381", "bw6_761"]


def _rand(rng, r, count):
    return [int.from_bytes(rng.bytes(64), "little") % r for _ in range(count)]


def _agree(polys, points, gamma, z, r):
    w_ref, claimed_ref, wp_ref = sm.reference_batch_open(polys, points, gamma, z, r)
    w, claimed, wp = sm.chain_batch_open(polys, points, gamma, z, r)
    maxlen = max(len(p) for p in polys)
    total = max(maxlen, max(len(s) for s in points) + 1) + sum(len(s) for s in points)
    assert len(w) == maxlen and len(wp) == maxlen - 1 and len(wp_ref) == total - 1
    assert sm.strip(w) == sm.strip(w_ref)
    assert claimed == claimed_ref
    assert wp + [0] * (len(wp_ref) - len(wp)) == wp_ref  # the reference's padding above the true degree is zero
    assert claimed == [[sm.eval_poly(f, s, r) for s in pts] for f, pts in zip(polys, points)]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_two_polynomials_every_length_and_set_size(gm, curve, shared):
    r = gm.CURVES[curve].r
    rng = rng_for(0x5B10, CURVES.index(curve), int(shared))
    gamma, z = _rand(rng, r, 2)
    pool = [0, 1, r - 1] + _rand(rng, r, 5)
    coeffs = _rand(rng, r, 24)
    for n0, m0, n1, m1 in itertools.product(range(1, 13), range(1, 4), range(1, 13), range(1, 4)):
        order = list(rng.permutation(len(pool)))
        s0 = [pool[i] for i in order[:m0]]
        s1 = [pool[i] for i in order[m0:m0 + m1]]
        if shared:
            s1[0] = s0[-1]  # equal points in different sets are legal
        _agree([coeffs[:n0], coeffs[12:12 + n1]], [s0, s1], gamma, z, r)


@pytest.mark.parametrize("curve", CURVES)
def test_three_polynomials_and_edge_challenges(gm, curve):
    r = gm.CURVES[curve].r
    rng = rng_for(0x5B11, CURVES.index(curve))
    pts = _rand(rng, r, 9)
    for lens, sizes in (((1, 1, 1), (1, 1, 1)), ((2, 12, 3), (3, 2, 3)), ((7, 1, 4), (1, 3, 2)), ((12, 12, 12), (3, 3, 3))):
        polys = [_rand(rng, r, n) for n in lens]
        points, at = [], 0
        for m in sizes:
            points.append(pts[at:at + m])
            at += m
        points[2][0] = points[0][0]
        for gamma, z in ((_rand(rng, r, 1)[0], _rand(rng, r, 1)[0]), (0, 0), (1, r - 1), (_rand(rng, r, 1)[0], points[1][0])):
            _agree(polys, points, gamma, z, r)  # the last z is a root of Z_T: L and w' are still defined


def test_degenerate_form_is_kzg_open():
    """k = 1 and one point: w is dividePolyByXminusA(f) and the claimed value is f(a)"""
    r = (1 << 61) - 1
    f, a = [5, 0, 7, 11, 3], 123456789
    w, claimed = sm.chain_open_w([f], [[a]], 99, r)
    h, fa = sm.divide_by_x_minus_a(f, a, r)
    assert w == h + [0] and claimed == [[fa]]
