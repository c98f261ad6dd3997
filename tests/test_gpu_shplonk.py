"""shplonk.BatchOpen on the device (gmsm_shplonk.h through include/gmsm.h and gnark-crypto_amd/shplonk.py), every curve's G1:
  - OpenW's w and claimed values and OpenWPrime's W' equal the reference-as-written model (tests/shplonk_model.py) limb for
    limb, W and W' equal ResidentBases.MultiExp of the model's w and w'; unequal lengths with an empty quotient, a point
    shared between sets, points from {0, 1, r - 1, random}; over plain bases and over window tables; 2^16 + 1 on BN254
  - k = 1 with one point is kzg.Open
  - over an SRS [alpha^i]G, W = [w(alpha)]G and W' = [L(alpha) / (alpha - z)]G with w(alpha), L(alpha) from the definitions
  - device-pointer inputs made on a torch stream give the same bits, d_out_w feeds open_wprime_device, inputs unmodified
  - every refusal of the ABI with its text, the size condition at its edge"""
import numpy as np
import pytest

import shplonk_model as sm
from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
ERR_SIZE = "invalid polynomial size (larger than SRS or == 0)"
LENS, SIZES = (2, 33, 2049, 4097), (3, 1, 2, 3)  # 4097: two tiles of the scan at that length's lane width; 2049: one tile + one lane


def ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    raw = a.reshape(-1, a.shape[-1]).astype("<u8").tobytes()
    w = 8 * a.shape[-1]
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def limbs(vals, nl):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(nl)] for v in vals], dtype=np.uint64).reshape(-1, nl)


def true(c, a):
    """Montgomery limbs -> true values"""
    rinv = pow(c.fr_R, -1, c.r)
    return [x * rinv % c.r for x in ints(a)]


def mont(c, vals):
    """true values -> Montgomery limbs"""
    return limbs([v % c.r * c.fr_R % c.r for v in vals], c.fr_limbs)


def rand_true(c, rng, n):
    return true(c, random_field_limbs(rng, c.r, c.fr_limbs, n))


def _bases(gm, curve, n):
    g = gm.G1Affine(curve)
    return g, g.generate_points(n, 0x5EED, 0xA11)


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_CASES = {}


def parity_case(gm, curve):
    """inputs (Montgomery limbs) and the reference-as-written model's outputs (true values), computed once per curve"""
    if curve not in _CASES:
        c = gm.CURVES[curve]
        rng = rng_for(0x5B20, CURVES.index(curve))
        ra, rb_, rc = rand_true(c, rng, 3)
        points = [[0, 1, ra], [c.r - 1], [rb_, 0], [1, c.r - 1, rc]]  # 0, 1 and r - 1 each sit in two sets
        polys = [rand_true(c, rng, n) for n in LENS]
        gamma, z = rand_true(c, rng, 2)
        w, claimed, wprime = sm.reference_batch_open(polys, points, gamma, z, c.r)
        _CASES[curve] = dict(polys=[mont(c, p) for p in polys], points=[mont(c, s) for s in points], gamma=mont(c, [gamma])[0],
                             z=mont(c, [z])[0], w=w, claimed=claimed, wprime=wprime)
    return _CASES[curve]


def check_against_model(gm, c, g, rb, case):
    polys, points = case["polys"], case["points"]
    before = [p.copy() for p in polys]
    maxlen = max(p.shape[0] for p in polys)
    claimed, w, W = gm.shplonk.OpenW(polys, points, case["gamma"], rb)
    assert w.shape == (maxlen, c.fr_limbs)
    assert true(c, w) == (case["w"] + [0] * maxlen)[:maxlen] and not any(case["w"][maxlen:])
    assert [true(c, v) for v in claimed] == case["claimed"]
    jac, err = rb.MultiExp(mont(c, case["w"][:maxlen]))
    assert err is None and (W == g.jac_to_affine(jac)).all()
    WP = gm.shplonk.OpenWPrime(polys, points, claimed, case["gamma"], w, case["z"], rb)
    assert not any(case["wprime"][maxlen - 1:])  # the reference's padding
    jac, err = rb.MultiExp(mont(c, case["wprime"][:maxlen - 1]))
    assert err is None and (WP == g.jac_to_affine(jac)).all()
    W2, WP2, claimed2 = gm.shplonk.BatchOpen(polys, points, case["gamma"], lambda got: case["z"] if (got == W).all() else None, rb)
    assert (W2 == W).all() and (WP2 == WP).all() and all((a == b).all() for a, b in zip(claimed, claimed2))
    assert all((p == b).all() for p, b in zip(polys, before))


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_matches_the_reference_model(gm, curve, tables):
    c = gm.CURVES[curve]
    g, pts = _bases(gm, curve, 5000)
    rb = g.register_bases(points=pts)
    try:
        if tables:
            rb.precompute(0)
        with gm.options(tables=2) if tables else _null():
            check_against_model(gm, c, g, rb, parity_case(gm, curve))
    finally:
        rb.release()


def test_matches_the_reference_model_other_lane_width(gm):
    """2^16 + 1 coefficients take the scan's 16-coefficient lanes (BN254 only: the kernels are templates of the field)"""
    curve = "bn254"
    c = gm.CURVES[curve]
    rng = rng_for(0x5B21)
    lens = ((1 << 16) + 1, 100)
    pa, pb, pc = rand_true(c, rng, 3)
    points = [[pa, pb], [pc]]
    polys = [rand_true(c, rng, n) for n in lens]
    gamma, z = rand_true(c, rng, 2)
    w, claimed, wprime = sm.reference_batch_open(polys, points, gamma, z, c.r)
    case = dict(polys=[mont(c, p) for p in polys], points=[mont(c, s) for s in points], gamma=mont(c, [gamma])[0], z=mont(c, [z])[0],
                w=w, claimed=claimed, wprime=wprime)
    g, pts = _bases(gm, curve, lens[0] + 3 - 1)
    rb = g.register_bases(points=pts)
    try:
        check_against_model(gm, c, g, rb, case)
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_one_polynomial_one_point_is_kzg_open(gm, curve):
    c = gm.CURVES[curve]
    rng = rng_for(0x5B22, CURVES.index(curve))
    g, pts = _bases(gm, curve, 3000)
    rb = g.register_bases(points=pts)
    try:
        f = random_field_limbs(rng, c.r, c.fr_limbs, 2500)
        a, gamma = random_field_limbs(rng, c.r, c.fr_limbs, 2)
        value, H = gm.kzg.Open(f, a, rb)
        claimed, w, W = gm.shplonk.OpenW([f], [a.reshape(1, -1)], gamma, rb)
        assert (W == H).all() and (claimed[0][0] == value).all()
        h, _ = gm.kzg.DividePolyByXMinusA(curve, f, a)
        assert (w[:-1] == h).all() and (w[-1] == 0).all()
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_over_known_alpha(gm, oracle_mod, curve):
    """independent of the model: over the SRS [alpha^i]G, W = [w(alpha)]G with w(alpha) = sum_i gamma^i (f_i(alpha) - r_i(alpha)) /
    Z_(S_i)(alpha), and W' = [w'(alpha)]G with (alpha - z) w'(alpha) = L(alpha), everything from the definitions in the field"""
    c = gm.CURVES[curve]
    r = c.r
    rng = rng_for(0x5B23, CURVES.index(curve))
    alpha = rand_true(c, rng, 1)[0]
    n = 400
    g = gm.G1Affine(curve)
    gen = np.array(g.generate_points(1, 0xC0FFEE, 0xBEEF)[0], dtype=np.uint64)
    srs = g.BatchScalarMultiplication(gen, mont(c, [pow(alpha, i, r) for i in range(n)]))
    rb = g.register_bases(points=srs)
    try:
        lens, sizes = (7, 300, 129), (2, 1, 3)
        polys = [rand_true(c, rng, m) for m in lens]
        pool = rand_true(c, rng, 5)
        points = [pool[0:2], pool[2:3], [pool[3], pool[0], pool[4]]]  # pool[0] in two sets
        assert tuple(len(s) for s in points) == sizes
        gamma, z = rand_true(c, rng, 2)
        claimed, w, W = gm.shplonk.OpenW([mont(c, p) for p in polys], [mont(c, s) for s in points], mont(c, [gamma])[0], rb)
        WP = gm.shplonk.OpenWPrime([mont(c, p) for p in polys], [mont(c, s) for s in points], claimed, mont(c, [gamma])[0], w,
                                   mont(c, [z])[0], rb)
        ev = lambda f, x: sum(co * pow(x, i, r) for i, co in enumerate(f)) % r

        def lagrange_at(s, y, x):  # the interpolant of (s_j, y_j) at x, from the Lagrange formula
            tot = 0
            for j in range(len(s)):
                num = den = 1
                for l in range(len(s)):
                    if l != j:
                        num, den = num * (x - s[l]) % r, den * (s[j] - s[l]) % r
                tot += y[j] * num * pow(den, -1, r)
            return tot % r

        def vanish(s, x):
            v = 1
            for a in s:
                v = v * (x - a) % r
            return v
        values = [[ev(f, a) for a in s] for f, s in zip(polys, points)]
        assert [true(c, v) for v in claimed] == values
        all_points = [a for s in points for a in s]
        w_alpha = sum(pow(gamma, i, r) * (ev(f, alpha) - lagrange_at(s, y, alpha)) * pow(vanish(s, alpha), -1, r)
                      for i, (f, s, y) in enumerate(zip(polys, points, values))) % r
        l_alpha = -vanish(all_points, z) * w_alpha
        for i, (f, s, y) in enumerate(zip(polys, points, values)):
            others = [a for l, t in enumerate(points) if l != i for a in t]
            l_alpha += pow(gamma, i, r) * vanish(others, z) * (ev(f, alpha) - lagrange_at(s, y, z))
        wp_alpha = l_alpha * pow(alpha - z, -1, r) % r
        o = oracle_mod.Oracle(curve, "g1")
        for got, scalar in ((W, w_alpha), (WP, wp_alpha)):
            exp = o.msm_affine(gen.reshape(1, -1), mont(c, [scalar]), nthreads=1)
            assert (got == np.asarray(exp).reshape(got.shape)).all()
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointers_on_a_torch_stream(gm, curve):
    import torch
    c = gm.CURVES[curve]
    case = parity_case(gm, curve)
    g, pts = _bases(gm, curve, 5000)
    rb = g.register_bases(points=pts)
    try:
        polys, points = case["polys"], case["points"]
        lens = [p.shape[0] for p in polys]
        flat = np.concatenate(polys)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            src = torch.from_numpy(flat.view(np.int64).copy()).cuda(non_blocking=False)
            d = src * 1  # produced by a kernel on s
            d_w = torch.full((max(lens) * c.fr_limbs,), -1, dtype=torch.int64, device="cuda")
            claimed, W = gm.shplonk.open_w_device(d.data_ptr(), lens, points, case["gamma"], rb, d_w.data_ptr(), s.cuda_stream)
            WP = gm.shplonk.open_wprime_device(d.data_ptr(), lens, points, claimed, case["gamma"], d_w.data_ptr(), case["z"], rb,
                                               s.cuda_stream)
        s.synchronize()
        hc, hw, hW = gm.shplonk.OpenW(polys, points, case["gamma"], rb)
        hWP = gm.shplonk.OpenWPrime(polys, points, hc, case["gamma"], hw, case["z"], rb)
        assert all((a == b).all() for a, b in zip(claimed, hc)) and (W == hW).all() and (WP == hWP).all()
        assert (d_w.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == hw).all()
        assert (d.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == flat).all()  # inputs unchanged
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_refusals(gm, curve):
    c = gm.CURVES[curve]
    rng = rng_for(0x5B24, CURVES.index(curve))
    g, pts = _bases(gm, curve, 64)
    rb = g.register_bases(points=pts)
    g2 = gm.G2Affine(curve)
    rb2 = g2.register_bases(points=g2.generate_points(64, 0x5EED, 0xA11))
    el = lambda n: random_field_limbs(rng, c.r, c.fr_limbs, n)
    f, s, gamma, z = el(10), el(2), el(1)[0], el(1)[0]
    w = np.zeros((10, c.fr_limbs), dtype=np.uint64)

    def both(polys, points, bases, text, claimed=None, w_=w):
        claimed = claimed if claimed is not None else [np.zeros_like(p) for p in points]
        with pytest.raises(ValueError) as e:
            gm.shplonk.OpenW(polys, points, gamma, bases)
        assert text in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            gm.shplonk.OpenWPrime(polys, points, claimed, gamma, w_, z, bases)
        assert text in str(e.value), str(e.value)
    try:
        both([], [], rb, "no polynomial", w_=w[:0])
        both([f], [s], rb2, "shplonk opens over G1 bases only")

        class Unknown:
            handle, group = 1 << 40, g
        both([f], [s], Unknown(), "unknown bases handle")
        both([f, f[:0]], [s, s], rb, "polynomial 1 is empty")
        both([f, f], [s, s[:0]], rb, "polynomial 1 has no opening point")
        both([f, f], [s, np.stack([s[0], s[1], s[0]])], rb, "set 1 holds the same point twice (points 0 and 2)")
        claimed, w1, _ = gm.shplonk.OpenW([f, f], [s, s], gamma, rb)  # equal points in different sets are legal
        gm.shplonk.OpenWPrime([f, f], [s, s], claimed, gamma, w1, z, rb)
        with pytest.raises(ValueError, match="number of digests should be equal to the number of points"):
            gm.shplonk.OpenW([f, f], [s], gamma, rb)
        L = gm._lib.load()  # pointer pairs: neither / both
        import ctypes
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        lens, npts, out, jac = (ctypes.c_size_t * 1)(10), (ctypes.c_size_t * 1)(2), np.zeros_like(s), np.zeros(g.jac_limbs, dtype=np.uint64)
        assert L.gmsm_shplonk_open_w(rb.handle, P(f), None, lens, 1, P(s), npts, P(gamma), None, P(out), None, None, P(jac)) == gm._lib.GMSM_ERR_ARG
        assert "exactly one of out_w (host) / d_out_w (device)" in gm._lib.last_error()
        assert L.gmsm_shplonk_open_wprime(rb.handle, P(f), None, lens, 1, P(s), npts, P(out), P(gamma), P(w), P(w), P(z), None,
                                          P(jac)) == gm._lib.GMSM_ERR_ARG
        assert "exactly one of w (host) / d_w (device)" in gm._lib.last_error()
    finally:
        rb.release()
        rb2.release()


@pytest.mark.parametrize("curve", CURVES)
def test_size_condition_at_its_edge(gm, curve):
    """the reference commits wPrime over maxSizePolys + sum m_i - 1 coefficients: a key one point short is refused"""
    c = gm.CURVES[curve]
    rng = rng_for(0x5B25, CURVES.index(curve))
    el = lambda n: random_field_limbs(rng, c.r, c.fr_limbs, n)
    gamma, z = el(1)[0], el(1)[0]
    # maxSizePolys from the longest polynomial, and from the largest set (m + 1 > every length)
    for lens, sizes in (((40, 7), (2, 3)), ((2, 3), (4, 1))):
        polys, points = [el(n) for n in lens], [el(m) for m in sizes]
        need = max(max(lens), max(sizes) + 1) + sum(sizes) - 1
        g, pts = _bases(gm, curve, need)
        short, exact = g.register_bases(points=pts[:need - 1]), g.register_bases(points=pts)
        try:
            w = np.zeros((max(lens), c.fr_limbs), dtype=np.uint64)
            with pytest.raises(ValueError) as e:
                gm.shplonk.OpenW(polys, points, gamma, short)
            assert str(e.value) == ERR_SIZE
            with pytest.raises(ValueError) as e:
                gm.shplonk.OpenWPrime(polys, points, [np.zeros_like(p) for p in points], gamma, w, z, short)
            assert str(e.value) == ERR_SIZE
            claimed, w, W = gm.shplonk.OpenW(polys, points, gamma, exact)
            gm.shplonk.OpenWPrime(polys, points, claimed, gamma, w, z, exact)
            tr = lambda a: true(c, a)
            mw, mclaimed, _ = sm.reference_batch_open([tr(p) for p in polys], [tr(s) for s in points], tr(gamma)[0], tr(z)[0], c.r)
            assert [tr(v) for v in claimed] == mclaimed and sm.strip(tr(w)) == sm.strip(mw)
        finally:
            short.release()
            exact.release()
