"""iop.Polynomial and iop.DivideByXMinusOne on the device (gnark-crypto_amd/iop.py over gmsm_iop_to_basis, gmsm_iop_evaluate,
gmsm_iop_divide_by_x_minus_one): every output limb for limb against the big-int model of tests/iop_poly_model.py (the
reference's loops and its conversion switch, pinned by tests/test_iop_poly_model.py), for the three scalar fields:
  - the 18 (form, target) conversions at cardinality 1, 2, 8 and 2^11 (the first size with a second FFT pass), len < cardinality
    at (5, 8), (2^11 - 3, 2^11) and len == 0 over a tail of non-zero garbage, host pointers and device pointers on a torch stream
  - Evaluate in the Lagrange bases: one tile / several tiles / a second round of the partial sums (default lanes: a tile is
    2048 coefficients, 1024 for BW6-761's 48-byte elements; GMSM_OPT_POLY_LANE_BITS = 1: 256), k = 1 and k = 3 with mixed
    layouts, x random, 0, on the domain (0, as in the reference), cosets g and 0, shifts 0..5
  - Evaluate in Canonical basis in both layouts, a blinded polynomial with a shift, shift 6 refused
  - DivideByXMinusOne for rho = 1 .. 2^11, both layouts, shifts, host and device, input unchanged, overlap refused, cached table
  - the reference's TestDivideByXMinusOne end to end on the device at n = 8 and n = 2^9
  - four threads on one pair of domains"""
import ctypes
import threading

import numpy as np
import pytest

import iop_model as M
import iop_poly_model as P
from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
CAN, LAG, COS = P.CANONICAL, P.LAGRANGE, P.LAGRANGE_COSET
REG, REV = P.REGULAR, P.BIT_REVERSE
FORMS = [(b, l) for b in (CAN, LAG, COS) for l in (REG, REV)]
LAYOUTS3 = [REG, REV, REG]
U32P = ctypes.POINTER(ctypes.c_uint32)
_VEC = {}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def vector(gm, curve, tag, count):
    """count random elements, made once per (curve, tag, count): (limbs, read-only; true values)"""
    key = (curve, tag, count)
    if key not in _VEC:
        c = gm.CURVES[curve]
        limbs = random_field_limbs(rng_for(0x10C0, CURVES.index(curve), tag, count), c.r, c.fr_limbs, count)
        limbs.setflags(write=False)
        _VEC[key] = (limbs, M.from_limbs(c, limbs))
    return _VEC[key]


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda() * 1  # produced by a kernel on the current stream


def download(c, t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs)


# ------------------------------------------------------------------ conversions
def run_to_basis(gm, d, limbs, length, form, target, device):
    """the C entry on a buffer of cardinality elements whose tail [length, cardinality) holds non-zero garbage"""
    import torch
    c, lib = d.curve, gm._lib.load()
    buf = np.full((d.Cardinality, c.fr_limbs), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    buf[:length] = limbs[:length]
    out_layout = ctypes.c_int(0)
    if not device:
        rc = lib.gmsm_iop_to_basis(d.handle, _p(buf), None, length, form[0], form[1], target, None, ctypes.byref(out_layout))
        assert rc == 0, lib.gmsm_last_error().decode()
        return buf, out_layout.value
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = upload(buf)
        layout = gm.iop.to_basis_device(d, t.data_ptr(), length, form, target, s.cuda_stream)
    s.synchronize()
    return download(c, t), layout


@pytest.mark.parametrize("card", [1, 2, 8, 1 << 11])
@pytest.mark.parametrize("curve", CURVES)
def test_conversions_against_the_model(gm, curve, card):
    c = gm.CURVES[curve]
    limbs, vals = vector(gm, curve, 1, card)
    md = P.Domain(c, card)
    d = gm.fft.NewDomain(curve, card)
    try:
        lens = {1: [1, 0], 2: [2], 8: [8, 5, 0], 1 << 11: [1 << 11, (1 << 11) - 3]}[card]
        for length in lens:
            for form in FORMS:
                for target in (LAG, CAN, COS):
                    exp = P.TO[target](P.Polynomial(vals[:length], *form), md)
                    assert len(exp.coefficients) == card
                    want = M.to_limbs(c, exp.coefficients)
                    for device in (False, True):
                        got, layout = run_to_basis(gm, d, limbs, length, form, target, device)
                        assert layout == exp.layout, (length, form, target, device)
                        assert (got == want).all(), (length, form, target, device)
    finally:
        d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_polynomial_mirror(gm, curve):
    """the reference's names through the mirror: grow, the coset, clones, GetCoeff, layouts, the ratio builders' triple"""
    iop = gm.iop
    c = gm.CURVES[curve]
    limbs, vals = vector(gm, curve, 2, 8)
    md = P.Domain(c, 8)
    d = gm.fft.NewDomain(curve, 8)
    try:
        p = iop.NewPolynomial(curve, limbs[:5].copy(), iop.Form(CAN, REG))
        assert (p.Size(), p.Basis, p.Layout) == (5, CAN, REG) and (p.coset == 0).all()
        shallow, deep = p.ShallowClone(), p.Clone()
        assert shallow.Coefficients() is p.Coefficients() and deep.Coefficients() is not p.Coefficients()
        assert p.ToLagrangeCoset(d) is p
        exp = P.to_lagrange_coset(P.Polynomial(vals[:5], CAN, REG), md)
        assert (p.Basis, p.Layout, p.Size()) == (COS, REV, 5) and (p.Coefficients() == M.to_limbs(c, exp.coefficients)).all()
        assert (p.coset == d.FrMultiplicativeGen).all()
        assert (deep.Coefficients() == limbs[:5]).all() and deep.Basis == CAN
        coefs, basis, layout = p  # what BuildRatio* take
        assert coefs is p.Coefficients() and (basis, layout) == (COS, REV)
        p.ToRegular()
        assert p.Layout == REG and (p.Coefficients() == M.to_limbs(c, P.to_regular(exp).coefficients)).all()
        p.SetSize(8)
        p.Shift(1)
        for i in (0, 3, 7):
            assert (p.GetCoeff(i) == p.Coefficients()[(i + 1) % 8]).all()
        p.ToBitReverse()
        for i in (0, 3, 7):
            assert (p.GetCoeff(i) == M.to_limbs(c, [exp.coefficients[(i + 1) % 8]])[0]).all()
        again = p.ToLagrangeCoset(d)  # already there: nothing but the coset is touched
        assert again.Layout == REV and (again.coset == d.FrMultiplicativeGen).all()
    finally:
        d.release()


# ------------------------------------------------------------------ Evaluate
def evaluate(gm, curve, limbs, k, length, size, basis, layouts, shift, coset, x, device=False):
    import torch
    c, lib = gm.CURVES[curve], gm._lib.load()
    xl = M.to_limbs(c, [x])[0]
    cl = None if coset is None else M.to_limbs(c, [coset])[0]
    if device:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = upload(limbs[:k * length])
            out = gm.iop.evaluate_device(curve, t.data_ptr(), k, length, size, basis, layouts, shift, cl, xl, s.cuda_stream)
        assert (download(c, t) == limbs[:k * length]).all()
        return out
    lay = np.array(layouts, dtype=np.uint32)
    out = np.zeros((k, c.fr_limbs), dtype=np.uint64)
    rc = lib.gmsm_iop_evaluate(gm._lib.GROUP_IDS[(curve, "g1")], _p(limbs), None, k, length, size, basis, lay.ctypes.data_as(U32P), shift,
                               None if cl is None else _p(cl), _p(xl), None, _p(out))
    assert rc == 0, lib.gmsm_last_error().decode()
    return out


def model_values(c, vals, k, length, size, basis, layouts, shift, coset, x):
    out = []
    for j in range(k):
        p = P.Polynomial(vals[j * length:(j + 1) * length], basis, layouts[j])
        p.shift, p.size, p.coset = shift, size, coset or 0
        out.append(P.evaluate(c, p, x))
    return M.to_limbs(c, out)


def check(gm, curve, length, k, basis, x, shift=0, size=None, coset=None, device=False, layouts=None):
    c = gm.CURVES[curve]
    limbs, vals = vector(gm, curve, 3, (3 if length <= 1 << 14 else 1) * length)  # beyond 2^14: k = 1
    layouts = layouts or LAYOUTS3[:k]
    size = size or length
    got = evaluate(gm, curve, limbs, k, length, size, basis, layouts, shift, coset, x, device)
    want = model_values(c, vals, k, length, size, basis, layouts, shift, coset, x)
    assert (got == want).all(), (length, k, basis, shift, size, coset, device)
    return got


# (poly_lane_bits, len): default lanes put 2048 coefficients in a tile (1024 for BW6-761), lanes of one element 256
LAGRANGE_SHAPES = [(0, 1), (0, 2), (0, 4), (0, 256), (0, 512), (0, 1024), (0, 2048), (0, 4096), (1, 256), (1, 512)]


@pytest.mark.parametrize("lanes,length", LAGRANGE_SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_evaluate_lagrange_against_the_model(gm, forced_options, curve, lanes, length):
    c = gm.CURVES[curve]
    r = c.r
    forced_options(poly_lane_bits=lanes)
    rng = rng_for(0x10C1, CURVES.index(curve), length)
    rand = lambda: int.from_bytes(rng.bytes(64), "little") % r
    w, g = M.generator(c, length), c.fr_mult_gen
    tile = 256 if lanes else 1024 if curve == "bw6_761" else 2048
    check(gm, curve, length, 1, LAG, rand())
    check(gm, curve, length, 3, LAG, rand(), device=True)
    check(gm, curve, length, 3, LAG, 0)
    on_domain = {0, length // 2, length - 1}
    if length > tile:
        on_domain |= {tile - 1, tile}  # one tile's last index, the next tile's first
    for j in sorted(on_domain):
        got = check(gm, curve, length, 3, LAG, pow(w, j, r))
        assert (got == 0).all()  # the reference's answer, not the interpolated value
        got = check(gm, curve, length, 1, COS, g * pow(w, j, r) % r, coset=g, layouts=[REV])
        assert (got == 0).all()
    check(gm, curve, length, 3, COS, rand(), coset=g)
    x = rand()
    got = check(gm, curve, length, 3, COS, x, coset=0)  # never went through ToLagrangeCoset: evaluated at 0
    assert (got == check(gm, curve, length, 3, LAG, 0)).all()
    for shift in range(6):
        check(gm, curve, length, 3 if shift == 1 else 1, LAG, x, shift=shift, size=length)
        check(gm, curve, length, 1, COS, x, shift=shift, size=max(length // 4, 1), coset=g, layouts=[REV])


@pytest.mark.parametrize("lanes,length", [(0, 1 << 14), (1, 1 << 14)])
@pytest.mark.parametrize("curve", CURVES)
def test_evaluate_lagrange_many_tiles(gm, forced_options, curve, lanes, length):
    """8 (16 for BW6-761) and 64 tiles"""
    c = gm.CURVES[curve]
    forced_options(poly_lane_bits=lanes)
    rng = rng_for(0x10C2, CURVES.index(curve), lanes)
    x = int.from_bytes(rng.bytes(64), "little") % c.r
    check(gm, curve, length, 3, LAG, x, device=bool(lanes))
    check(gm, curve, length, 1, COS, x, shift=2, size=length // 4, coset=c.fr_mult_gen, layouts=[REV])
    got = check(gm, curve, length, 1, LAG, pow(M.generator(c, length), 2048 if not lanes else 255, c.r))
    assert (got == 0).all()


@pytest.mark.parametrize("lanes,length", [(0, 1 << 17), (1, 1 << 16), (1, 1 << 17)])
def test_evaluate_lagrange_partial_sum_rounds(gm, forced_options, lanes, length):
    """BN254 only: 2^17 with default lanes, and lanes of one element at 256 tiles (one round of the final sum's lanes) and 512
    (two)"""
    c = gm.CURVES["bn254"]
    forced_options(poly_lane_bits=lanes)
    x = int.from_bytes(rng_for(0x10C3, length, lanes).bytes(64), "little") % c.r
    check(gm, "bn254", length, 1, LAG, x, layouts=[REV] if lanes else [REG])


@pytest.mark.parametrize("curve", CURVES)
def test_evaluate_canonical_against_the_model(gm, curve):
    c = gm.CURVES[curve]
    lib = gm._lib.load()
    rng = rng_for(0x10C4, CURVES.index(curve))
    rand = lambda: int.from_bytes(rng.bytes(64), "little") % c.r
    for length in (1, 7, 256, 2049):
        check(gm, curve, length, 3, CAN, rand(), layouts=[REG] * 3, device=length == 256)
        check(gm, curve, length, 1, CAN, 0, layouts=[REG])
    for length in (256, 4096):
        check(gm, curve, length, 3, CAN, rand())  # Regular, BitReverse, Regular
        check(gm, curve, length, 1, CAN, rand(), layouts=[REV], device=True)
    for shift in range(6):
        check(gm, curve, 11, 1, CAN, rand(), shift=shift, size=8, layouts=[REG])  # a blinded polynomial: len 11, size 8
    check(gm, curve, 256, 1, CAN, rand(), shift=5, size=64, layouts=[REV])
    # shift 6: the reference evaluates at 0 (an element it never initialised); refused here
    limbs, _ = vector(gm, curve, 3, 33)
    lay = np.array([REG], dtype=np.uint32)
    out = np.zeros((1, c.fr_limbs), dtype=np.uint64)
    x = M.to_limbs(c, [5])[0]
    rc = lib.gmsm_iop_evaluate(gm._lib.GROUP_IDS[(curve, "g1")], _p(limbs), None, 1, 11, 8, CAN, lay.ctypes.data_as(U32P), 6, None, _p(x), None,
                               _p(out))
    assert rc == 4 and "shift 6 is outside 0..5" in lib.gmsm_last_error().decode() and (out == 0).all()
    p = gm.iop.NewPolynomial(curve, limbs[:11].copy(), gm.iop.Form(CAN, REG)).Shift(6)
    p.SetSize(8)
    with pytest.raises(ValueError, match="shift 6 is outside 0..5"):
        p.Evaluate(x)
    p.Shift(1)
    _, vals = vector(gm, curve, 3, 33)
    mp = P.Polynomial(vals[:11], CAN, REG)
    mp.shift, mp.size = 1, 8
    assert (p.Evaluate(x) == M.to_limbs(c, [P.evaluate(c, mp, 5)])[0]).all()
    # the G2 group id names the same scalar field
    rc = lib.gmsm_iop_evaluate(gm._lib.GROUP_IDS[(curve, "g2")], _p(limbs), None, 1, 11, 8, CAN, lay.ctypes.data_as(U32P), 1, None, _p(x), None,
                               _p(out))
    assert rc == 0 and (out[0] == p.Evaluate(x)).all()


# ------------------------------------------------------------------ DivideByXMinusOne
QUOTIENT_SHAPES = [(1, 1), (1, 4), (8, 32), (1 << 9, 1 << 11), (1 << 10, 1 << 10), (2, 1 << 12)]


@pytest.mark.parametrize("n,N", QUOTIENT_SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_divide_by_x_minus_one_against_the_model(gm, curve, n, N):
    import torch
    c = gm.CURVES[curve]
    iop = gm.iop
    limbs, vals = vector(gm, curve, 4, N)
    mdom = (P.Domain(c, n), P.Domain(c, N))
    doms = (gm.fft.NewDomain(curve, n), gm.fft.NewDomain(curve, N))
    try:
        for layout in (REG, REV):
            for shift in sorted({0, 1, n - 1}):  # the second and later calls on these domains read the cached table
                mp = P.Polynomial(vals, COS, layout)
                mp.size, mp.shift = n, shift
                mq = P.divide_by_x_minus_one(mp, mdom)
                want = M.to_limbs(c, mq.coefficients)
                a = iop.NewPolynomial(curve, limbs.copy(), iop.Form(COS, layout)).Shift(shift)
                a.SetSize(n)
                q = iop.DivideByXMinusOne(a, doms)
                assert (q.Basis, q.Layout, q.Size()) == (CAN, REG, n) and (q.Coefficients() == want).all(), (layout, shift)
                assert (a.Coefficients() == limbs).all()  # input unchanged
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    t = upload(limbs)
                    out = torch.empty_like(t)
                    iop.divide_by_x_minus_one_device(doms, t.data_ptr(), (COS, layout), shift, out.data_ptr(), s.cuda_stream)
                s.synchronize()
                assert (download(c, out) == want).all(), (layout, shift)
                assert (download(c, t) == limbs).all()
    finally:
        for d in doms:
            d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_divide_by_x_minus_one_refusals(gm, curve):
    import torch
    c = gm.CURVES[curve]
    lib = gm._lib.load()
    nl = c.fr_limbs
    n, N = 8, 32
    err = lambda: lib.gmsm_last_error().decode()
    other = CURVES[(CURVES.index(curve) + 1) % 3]
    doms = (gm.fft.NewDomain(curve, n), gm.fft.NewDomain(curve, N))
    foreign = gm.fft.NewDomain(other, n)
    div = lib.gmsm_iop_divide_by_x_minus_one
    try:
        big = np.zeros((2 * N, nl), dtype=np.uint64)
        for out in (big[:N], big[N - 1:2 * N - 1], big[1:N + 1]):
            assert div(doms[0].handle, doms[1].handle, _p(big), None, COS, REG, 0, None, _p(out), None) == 4
            assert err().endswith("the output overlaps an input (inputs are never modified)")
        assert div(doms[0].handle, doms[1].handle, _p(big), None, COS, REG, 0, None, _p(big[N:]), None) == 0  # adjacent
        dev = torch.zeros(2 * N * nl, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for ptr in (dev.data_ptr(), dev.data_ptr() + (N - 1) * nl * 8):
            assert div(doms[0].handle, doms[1].handle, None, dev.data_ptr(), COS, REV, 0, None, None, ptr) == 4
            assert err().endswith("the output overlaps an input (inputs are never modified)")
        out = big[N:]
        assert div(doms[1].handle, doms[0].handle, _p(big), None, COS, REG, 0, None, _p(out), None) == 4 and "larger than the big one" in err()
        assert div(foreign.handle, doms[1].handle, _p(big), None, COS, REG, 0, None, _p(out), None) == 4 and "different curves" in err()
        assert div(doms[0].handle, doms[1].handle, _p(big), None, LAG, REG, 0, None, _p(out), None) == 4
        assert err() == "the basis must be LagrangeCoset"
        with pytest.raises(ValueError) as e:
            gm.iop.DivideByXMinusOne(gm.iop.NewPolynomial(curve, big[:N], gm.iop.Form(CAN, REG)), doms)
        assert str(e.value) == "the basis must be LagrangeCoset"
        # to_basis: a vector longer than the domain
        lay = ctypes.c_int(0)
        assert lib.gmsm_iop_to_basis(doms[0].handle, _p(big), None, n + 1, CAN, REG, LAG, None, ctypes.byref(lay)) == 4
        assert "len 9 is larger than the domain's cardinality" in err()
    finally:
        for d in doms + (foreign,):
            d.release()


def quotient_identity(gm, curve, n):
    """TestDivideByXMinusOne (quotient_test.go:33-132) with every polynomial step on the device; the numerator h(a, b, c) on the
    big coset is the caller's own expression: built here with big ints"""
    c = gm.CURVES[curve]
    r = c.r
    iop = gm.iop
    N = P.next_power_of_two(3 * n)
    h = lambda x1, x2, x3: (x1 * x1 * x2 + x3 - x1 * x1 * x1) % r
    _, va = vector(gm, curve, 5, n)
    _, vb = vector(gm, curve, 6, n)
    vc = [(x * x * x - x * x * y) % r for x, y in zip(va, vb)]
    doms = (gm.fft.NewDomain(curve, n), gm.fft.NewDomain(curve, N))
    try:
        entries = []
        for v in (va, vb, vc):
            p = iop.NewPolynomial(curve, M.to_limbs(c, v), iop.Form(LAG, REG))
            p.ToCanonical(doms[0]).ToRegular().ToLagrangeCoset(doms[1]).ToRegular()
            assert (p.Basis, p.Layout, p.Size(), p.Coefficients().shape[0]) == (COS, REG, n, N)
            entries.append(p)
        on_coset = [M.from_limbs(c, e.Coefficients()) for e in entries]
        num = [0] * N
        for i in range(N):
            num[M.bit_reverse_index(i, N)] = h(on_coset[0][i], on_coset[1][i], on_coset[2][i])
        hp = iop.NewPolynomial(curve, M.to_limbs(c, num), iop.Form(COS, REV))
        hp.SetSize(n)
        q = iop.DivideByXMinusOne(hp, doms)
        x = int.from_bytes(rng_for(0x10C5, n).bytes(64), "little") % r
        xl = M.to_limbs(c, [x])[0]
        qx = M.from_limbs(c, q.Evaluate(xl))[0]
        abc = [M.from_limbs(c, e.ToCanonical(doms[1]).Evaluate(xl))[0] for e in entries]
        assert qx * (pow(x, n, r) - 1) % r == h(*abc)
        # and the entries are still the polynomials they were: degree < n, the given values on the small domain
        w = M.generator(c, n)
        e0 = entries[0].ToRegular()
        assert (e0.Coefficients()[n:] == 0).all()
        assert M.from_limbs(c, e0.Evaluate(M.to_limbs(c, [pow(w, 3 % n, r)])[0]))[0] == va[3 % n]
    finally:
        for d in doms:
            d.release()


@pytest.mark.parametrize("n", [8, 1 << 9])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_identity_end_to_end(gm, curve, n):
    quotient_identity(gm, curve, n)


@pytest.mark.parametrize("curve", CURVES)
def test_four_threads_on_one_pair_of_domains(gm, curve):
    c = gm.CURVES[curve]
    iop = gm.iop
    n, N = 1 << 9, 1 << 11
    limbs, vals = vector(gm, curve, 4, N)
    mdom = (P.Domain(c, n), P.Domain(c, N))
    x = 0x1234567 % c.r
    xl = M.to_limbs(c, [x])[0]
    jobs = [(REG, 0), (REV, 1), (REG, n - 1), (REV, 0)]
    want = []
    for layout, shift in jobs:
        mp = P.Polynomial(vals, COS, layout)
        mp.size, mp.shift = n, shift
        mq = P.divide_by_x_minus_one(mp, mdom)
        ml = P.to_lagrange(mq.clone(), mdom[1])
        want.append((M.to_limbs(c, mq.coefficients), M.to_limbs(c, ml.coefficients), M.to_limbs(c, [P.evaluate(c, mq, x)])[0]))
    doms = (gm.fft.NewDomain(curve, n), gm.fft.NewDomain(curve, N))
    try:
        errs = []

        def run(i):
            try:
                layout, shift = jobs[i]
                for _ in range(3):
                    a = iop.NewPolynomial(curve, limbs.copy(), iop.Form(COS, layout)).Shift(shift)
                    a.SetSize(n)
                    q = iop.DivideByXMinusOne(a, doms)
                    assert (q.Coefficients() == want[i][0]).all()
                    assert (q.Evaluate(xl) == want[i][2]).all()
                    lag = q.Clone().ToLagrange(doms[1])
                    assert lag.Layout == REV and (lag.Coefficients() == want[i][1]).all()
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
    finally:
        for d in doms:
            d.release()
