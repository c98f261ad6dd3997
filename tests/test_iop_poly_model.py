"""Pins tests/iop_poly_model.py (the big-int model the GPU tests compare against) without a GPU or the library:
  - Lagrange evaluation at len 1, 2, 8, 64 equals Horner on the coefficients of a naive O(n^2) inverse DFT at random x, is 0
    for x in the domain (the reference's answer), and the coset form equals evaluation at x / g
  - the properties of the reference's polynomial_test.go at size 8: the conversions round-trip through every form
    (TestRoundTrip), ToLagrange / ToCanonical / ToLagrangeCoset from each of the six forms give the naive evaluations in the
    layout the switch leaves (TestPutIn*Form), GetCoeff with a shift in both layouts (TestGetCoeff)
  - the reference's TestDivideByXMinusOne at n = 8, N = 32: the entries vanish under h = x1^2 x2 + x3 - x1^3 and
    q(x) (x^n - 1) = h(a(x), b(x), c(x)) at a random x"""
import random

import pytest

import iop_model as M
import iop_poly_model as P

CURVES = ["bn254", "bls12_381", "bw6_761"]
FORMS = [(b, l) for b in (P.CANONICAL, P.LAGRANGE, P.LAGRANGE_COSET) for l in (P.REGULAR, P.BIT_REVERSE)]


def horner(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def naive_inverse_dft(values, w, r):
    n = len(values)
    ninv, winv = pow(n, -1, r), pow(w, -1, r)
    return [sum(values[i] * pow(winv, i * k, r) for i in range(n)) * ninv % r for k in range(n)]


def in_form(c, coeffs, d, basis, layout):
    """the polynomial with these canonical coefficients (len = the domain's cardinality) in the given form, by definition"""
    n, r = d.cardinality, c.r
    if basis == P.CANONICAL:
        vals = list(coeffs)
    else:
        g = d.fr_multiplicative_gen if basis == P.LAGRANGE_COSET else 1
        vals = [horner(coeffs, g * pow(d.generator, i, r) % r, r) for i in range(n)]
    if layout == P.BIT_REVERSE:
        vals = [vals[M.bit_reverse_index(i, n)] for i in range(n)]
    p = P.Polynomial(vals, basis, layout)
    if basis == P.LAGRANGE_COSET:
        p.coset = d.fr_multiplicative_gen
    return p


@pytest.mark.parametrize("n", [1, 2, 8, 64])
@pytest.mark.parametrize("curve", CURVES)
def test_lagrange_evaluation(gm, curve, n):
    c = gm.CURVES[curve]
    r = c.r
    rnd = random.Random(n * 7 + CURVES.index(curve))
    d = P.Domain(c, n)
    values = [rnd.randrange(r) for _ in range(n)]
    coeffs = naive_inverse_dft(values, d.generator, r)
    for layout in (P.REGULAR, P.BIT_REVERSE):
        stored = values if layout == P.REGULAR else [values[M.bit_reverse_index(i, n)] for i in range(n)]
        p = P.Polynomial(stored, P.LAGRANGE, layout)
        for x in (rnd.randrange(r), 0):
            assert P.evaluate(c, p, x) == horner(coeffs, x, r)
        for j in {0, n // 2, n - 1}:
            assert P.evaluate(c, p, pow(d.generator, j, r)) == 0  # the reference's answer on the domain, not values[j]
        pc = P.Polynomial(stored, P.LAGRANGE_COSET, layout)
        pc.coset = d.fr_multiplicative_gen
        x = rnd.randrange(r)
        assert P.evaluate(c, pc, x) == horner(coeffs, x * pow(pc.coset, -1, r) % r, r)
        pc.coset = 0  # never went through ToLagrangeCoset: evaluated at 0
        assert P.evaluate(c, pc, x) == horner(coeffs, 0, r)
        # a shift multiplies x by Generator(size)^shift
        ps = P.Polynomial(stored, P.LAGRANGE, layout)
        ps.shift = 1
        x = rnd.randrange(r)
        assert P.evaluate(c, ps, x) == horner(coeffs, x * d.generator % r, r)
        pk = P.Polynomial(coeffs, P.CANONICAL, P.REGULAR)
        pk.shift, pk.size = 3, max(n // 4, 1)
        assert P.evaluate(c, pk, x) == horner(coeffs, x * pow(M.generator(c, pk.size), 3, r) % r, r)


@pytest.mark.parametrize("curve", CURVES)
def test_conversions_give_the_naive_evaluations(gm, curve):
    """TestPutInLagrangeForm / CanonicalForm / LagrangeCosetForm: from each of the six forms to each target"""
    c = gm.CURVES[curve]
    rnd = random.Random(0x10F + CURVES.index(curve))
    d = P.Domain(c, 8)
    coeffs = [rnd.randrange(c.r) for _ in range(8)]
    flip = {P.REGULAR: P.BIT_REVERSE, P.BIT_REVERSE: P.REGULAR}
    for basis, layout in FORMS:
        for target in (P.LAGRANGE, P.CANONICAL, P.LAGRANGE_COSET):
            p = P.TO[target](in_form(c, coeffs, d, basis, layout), d)
            steps = 0 if basis == target else 1 if P.CANONICAL in (basis, target) else 2
            out_layout = flip[layout] if steps == 1 else layout
            exp = in_form(c, coeffs, d, target, out_layout)
            assert (p.basis, p.layout) == (target, out_layout), (basis, layout, target)
            assert p.coefficients == exp.coefficients, (basis, layout, target)


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip_and_grow(gm, curve):
    c = gm.CURVES[curve]
    rnd = random.Random(0x20F + CURVES.index(curve))
    d = P.Domain(c, 8)
    coeffs = [rnd.randrange(c.r) for _ in range(8)]
    p = P.Polynomial(coeffs, P.CANONICAL, P.REGULAR)
    for target in (P.LAGRANGE_COSET, P.LAGRANGE, P.CANONICAL, P.LAGRANGE, P.LAGRANGE_COSET, P.CANONICAL):
        P.TO[target](p, d)
    assert P.to_regular(p).coefficients == coeffs and p.coset == d.fr_multiplicative_gen
    # grow: 5 coefficients on a domain of 8 are the polynomial with three zero coefficients appended, also for the identity
    short = P.to_lagrange(P.Polynomial(coeffs[:5], P.CANONICAL, P.REGULAR), d)
    assert short.coefficients == in_form(c, coeffs[:5] + [0, 0, 0], d, P.LAGRANGE, P.BIT_REVERSE).coefficients
    same = P.to_canonical(P.Polynomial(coeffs[:5], P.CANONICAL, P.BIT_REVERSE), d)
    assert same.coefficients == coeffs[:5] + [0, 0, 0] and same.layout == P.BIT_REVERSE


def test_get_coeff():
    """TestGetCoeff (polynomial_test.go:118-162)"""
    wp = P.Polynomial(list(range(8)), P.CANONICAL, P.REGULAR)
    wsp = wp.clone()
    wsp.shift = 1
    for _ in range(2):
        for i in range(8):
            assert P.get_coeff(wp, i) == i and P.get_coeff(wsp, i) == (i + 1) % 8
        P.to_bit_reverse(wp)
        P.to_bit_reverse(wsp)
    ext = P.Polynomial(list(range(32)), P.LAGRANGE_COSET, P.REGULAR)  # 8 coefficients on 32 points: a shift moves by rho = 4
    ext.size, ext.shift = 8, 3
    assert [P.get_coeff(ext, i) for i in (0, 1, 20, 31)] == [12, 13, 0, 11]


@pytest.mark.parametrize("curve", CURVES)
def test_divide_by_x_minus_one(gm, curve):
    """TestDivideByXMinusOne (quotient_test.go:33-132), n = 8, N = 32"""
    c = gm.CURVES[curve]
    r = c.r
    rnd = random.Random(0x30F + CURVES.index(curve))
    n = 8
    h = lambda x1, x2, x3: (x1 * x1 * x2 + x3 - x1 * x1 * x1) % r
    a = [rnd.randrange(r) for _ in range(n)]
    b = [rnd.randrange(r) for _ in range(n)]
    cc = [(x * x * x - x * x * y) % r for x, y in zip(a, b)]
    assert all(h(*t) == 0 for t in zip(a, b, cc))
    domains = (P.Domain(c, n), P.Domain(c, P.next_power_of_two(3 * n)))
    entries = []
    for v in (a, b, cc):
        p = P.Polynomial(v, P.LAGRANGE, P.REGULAR)
        P.to_regular(P.to_lagrange_coset(P.to_regular(P.to_canonical(p, domains[0])), domains[1]))
        assert len(p.coefficients) == 32 and p.size == 8
        entries.append(p)
    num = P.Polynomial([0] * 32, P.LAGRANGE_COSET, P.BIT_REVERSE)  # iop.Evaluate(f, nil, {LagrangeCoset, BitReverse}, entries...)
    num.size = entries[0].size
    for i in range(32):
        num.coefficients[M.bit_reverse_index(i, 32)] = h(*[P.get_coeff(e, i) for e in entries])
    with pytest.raises(ValueError, match="the basis must be LagrangeCoset"):
        P.divide_by_x_minus_one(P.Polynomial([0] * 32, P.LAGRANGE, P.REGULAR), domains)
    q = P.divide_by_x_minus_one(num, domains)
    assert (q.basis, q.layout, q.size, len(q.coefficients)) == (P.CANONICAL, P.REGULAR, 8, 32)
    x = rnd.randrange(r)
    for e in entries:
        P.to_canonical(e, domains[1])
    lhs = P.evaluate(c, q, x) * (pow(x, n, r) - 1) % r
    assert lhs == h(*[P.evaluate(c, e, x) for e in entries])
