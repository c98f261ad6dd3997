"""fflonk Fold, FoldAndCommit and BatchOpen on the device (gmsm_fflonk.h through include/gmsm.h and
gnark-crypto_amd/fflonk.py), every curve's G1. Four packs cover every index path of the three kernels:
  A  3 polynomials, t = 3, lengths (33, 2049, 1), points {random, 1}: odd t; one tile plus one lane of the scan; a
     length-1 member whose chain runs out
  B  5 polynomials, t = 6, lengths (4097, 2, 0, 700, 64), point {r - 1}: a padded slot; an empty member; two scan tiles
  C  1 polynomial, t = 1, length 2, points {0, 1, random}: z = 0 legal; the quotient is empty after two divisions
  D  2 polynomials, t = 2, lengths (1, 1), two random points: every chain empty; contributes nothing to w
  - Fold, FoldAndCommit, w, both sets of claimed values, W and W' equal the reference-as-written model
    (tests/fflonk_model.py), over plain bases and over window tables
  - fold_device + the existing shplonk entries on the extended sets give the same w, W, W' and inner claimed values
  - another lane width of the scan; device pointers on a torch stream; every refusal with its text; the size condition
    over the folded sizes at its edge"""
import itertools

import numpy as np
import pytest

import fflonk_model as fm
from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
ERR_SIZE = "invalid polynomial size (larger than SRS or == 0)"
PACK_LENS = ((33, 2049, 1), (4097, 2, 0, 700, 64), (2,), (1, 1))
KEY = 6 * 4097 + 19  # max t_i n_i + sum t_i m_i - 1 = 6 * 4097 + 18: one point to spare


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
        rng = rng_for(0xFF20, CURVES.index(curve))
        ra, rc, rd, re_ = rand_true(c, rng, 4)
        points = [[ra, 1], [c.r - 1], [0, 1, rc], [rd, re_]]  # the point 1 sits in two packs
        packs = [[rand_true(c, rng, n) for n in lens] for lens in PACK_LENS]
        assert [fm.next_divisor(len(p), c.r) for p in packs] == [3, 6, 1, 2]
        gamma, z = rand_true(c, rng, 2)
        w, claimed, folded_claimed, wprime = fm.reference_batch_open(packs, points, gamma, z, c.r, c.fr_mult_gen)
        _CASES[curve] = dict(packs=[[mont(c, p) for p in pack] for pack in packs], points=[mont(c, s) for s in points],
                             gamma=mont(c, [gamma])[0], z=mont(c, [z])[0], w=w, claimed=claimed, folded_claimed=folded_claimed,
                             wprime=wprime, folds=[fm.fold(p, c.r) for p in packs])
    return _CASES[curve]


def check_against_model(gm, c, g, rb, case, folds=True):
    packs, points = case["packs"], case["points"]
    before = [[p.copy() for p in pack] for pack in packs]
    maxfold = max(len(f) for f in case["folds"])
    if folds:
        for pack, want in zip(packs, case["folds"]):
            got = gm.fflonk.Fold(c.name, pack)
            assert got.shape == (len(want), c.fr_limbs) and true(c, got) == want  # limb for limb: both sides are canonical
            assert (got == mont(c, want)).all()
            jac, err = rb.MultiExp(mont(c, want))
            assert err is None and (gm.fflonk.FoldAndCommit(pack, rb) == g.jac_to_affine(jac)).all()
    claimed, folded_claimed, w, W = gm.fflonk.OpenW(packs, points, case["gamma"], rb)
    assert w.shape == (maxfold, c.fr_limbs)
    assert true(c, w) == (case["w"] + [0] * maxfold)[:maxfold] and not any(case["w"][maxfold:])
    for got, want, pack in zip(claimed, case["claimed"], packs):
        assert got.shape[:2] == (len(want), len(want[0])) and [true(c, row) for row in got] == want
        assert not got[len(pack):].any()  # the rows past the pack's size
    assert [true(c, v) for v in folded_claimed] == case["folded_claimed"]
    jac, err = rb.MultiExp(mont(c, case["w"][:maxfold]))
    assert err is None and (W == g.jac_to_affine(jac)).all()
    WP = gm.fflonk.OpenWPrime(packs, points, folded_claimed, case["gamma"], w, case["z"], rb)
    assert not any(case["wprime"][maxfold - 1:])  # the reference's padding
    jac, err = rb.MultiExp(mont(c, case["wprime"][:maxfold - 1]))
    assert err is None and (WP == g.jac_to_affine(jac)).all()
    W2, WP2, folded2, claimed2 = gm.fflonk.BatchOpen(packs, points, case["gamma"], lambda got: case["z"] if (got == W).all() else None, rb)
    assert (W2 == W).all() and (WP2 == WP).all()
    assert all((a == b).all() for a, b in zip(claimed, claimed2)) and all((a == b).all() for a, b in zip(folded_claimed, folded2))
    assert all((p == b).all() for pack, bpack in zip(packs, before) for p, b in zip(pack, bpack))


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_matches_the_reference_model(gm, curve, tables):
    c = gm.CURVES[curve]
    g, pts = _bases(gm, curve, KEY)
    rb = g.register_bases(points=pts)
    try:
        if tables:
            rb.precompute(0)
        with gm.options(tables=2) if tables else _null():
            check_against_model(gm, c, g, rb, parity_case(gm, curve))
    finally:
        rb.release()


def _extended(c, case):
    ts = [fm.next_divisor(len(p), c.r) for p in case["packs"]]
    return ts, [mont(c, fm.extend_set(true(c, s), t, c.r, c.fr_mult_gen)) for s, t in zip(case["points"], ts)]


@pytest.mark.parametrize("curve", CURVES)
def test_equals_shplonk_over_the_folded_polynomials(gm, curve):
    """no model: fold_device, then the merged shplonk entries over the folded polynomials and the extended sets"""
    import torch
    c = gm.CURVES[curve]
    case = parity_case(gm, curve)
    g, pts = _bases(gm, curve, KEY)
    rb = g.register_bases(points=pts)
    try:
        packs, points = case["packs"], case["points"]
        ts, ext = _extended(c, case)
        flens = [t * max(p.shape[0] for p in pack) for t, pack in zip(ts, packs)]
        stream = torch.cuda.current_stream().cuda_stream
        d_folded = torch.full((sum(flens) * c.fr_limbs,), -1, dtype=torch.int64, device="cuda")
        at = 0
        for pack, n in zip(packs, flens):
            d_pack = torch.from_numpy(np.concatenate(pack).view(np.int64).copy()).cuda()
            gm.fflonk.fold_device(curve, d_pack.data_ptr(), [p.shape[0] for p in pack], d_folded.data_ptr() + 8 * at * c.fr_limbs, stream)
            at += n
        d_w = torch.full((max(flens) * c.fr_limbs,), -1, dtype=torch.int64, device="cuda")
        s_claimed, sW = gm.shplonk.open_w_device(d_folded.data_ptr(), flens, ext, case["gamma"], rb, d_w.data_ptr(), stream)
        sWP = gm.shplonk.open_wprime_device(d_folded.data_ptr(), flens, ext, s_claimed, case["gamma"], d_w.data_ptr(), case["z"], rb, stream)
        claimed, folded_claimed, w, W = gm.fflonk.OpenW(packs, points, case["gamma"], rb)
        WP = gm.fflonk.OpenWPrime(packs, points, folded_claimed, case["gamma"], w, case["z"], rb)
        assert (d_w.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == w).all()
        assert all((a == b).all() for a, b in zip(s_claimed, folded_claimed))
        assert (sW == W).all() and (sWP == WP).all()
    finally:
        rb.release()


def test_other_lane_width(gm):
    """BN254 only (the kernels are templates of the field): 2^16 + 1 coefficients take the scan's 16-coefficient lanes, and
    pack A again with poly_lane_bits forced to 2-coefficient lanes (several tiles, the carry pass)"""
    curve = "bn254"
    c = gm.CURVES[curve]
    rng = rng_for(0xFF21)
    n = (1 << 16) + 1
    packs = [[rand_true(c, rng, n), rand_true(c, rng, n)]]
    points = [rand_true(c, rng, 1)]
    gamma, z = rand_true(c, rng, 2)
    w, claimed, folded_claimed, wprime = fm.reference_batch_open(packs, points, gamma, z, c.r, c.fr_mult_gen)
    case = dict(packs=[[mont(c, p) for p in pack] for pack in packs], points=[mont(c, s) for s in points], gamma=mont(c, [gamma])[0],
                z=mont(c, [z])[0], w=w, claimed=claimed, folded_claimed=folded_claimed, wprime=wprime, folds=[fm.fold(p, c.r) for p in packs])
    g, pts = _bases(gm, curve, 2 * n + 2 - 1)
    rb = g.register_bases(points=pts)
    try:
        check_against_model(gm, c, g, rb, case, folds=False)
        full = parity_case(gm, curve)
        packs_a, points_a = [[rand_true(c, rng, m) for m in PACK_LENS[0]]], [true(c, full["points"][0])]
        w, claimed, folded_claimed, wprime = fm.reference_batch_open(packs_a, points_a, gamma, z, c.r, c.fr_mult_gen)
        case_a = dict(packs=[[mont(c, p) for p in pack] for pack in packs_a], points=[full["points"][0]], gamma=case["gamma"], z=case["z"],
                      w=w, claimed=claimed, folded_claimed=folded_claimed, wprime=wprime, folds=[fm.fold(p, c.r) for p in packs_a])
        with gm.options(poly_lane_bits=2):
            check_against_model(gm, c, g, rb, case_a, folds=False)
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointers_on_a_torch_stream(gm, curve):
    import torch
    c = gm.CURVES[curve]
    case = parity_case(gm, curve)
    g, pts = _bases(gm, curve, KEY)
    rb = g.register_bases(points=pts)
    try:
        packs, points = case["packs"], case["points"]
        members = [p for pack in packs for p in pack]
        lens, pack_sizes = [p.shape[0] for p in members], [len(pack) for pack in packs]
        flat = np.concatenate(members)
        maxfold = max(len(f) for f in case["folds"])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            src = torch.from_numpy(flat.view(np.int64).copy()).cuda(non_blocking=False)
            d = src * 1  # produced by a kernel on s
            d_w = torch.full((maxfold * c.fr_limbs,), -1, dtype=torch.int64, device="cuda")
            claimed, folded_claimed, W = gm.fflonk.open_w_device(d.data_ptr(), lens, pack_sizes, points, case["gamma"], rb, d_w.data_ptr(),
                                                                 s.cuda_stream)
            WP = gm.fflonk.open_wprime_device(d.data_ptr(), lens, pack_sizes, points, folded_claimed, case["gamma"], d_w.data_ptr(), case["z"],
                                              rb, s.cuda_stream)
            # pack B alone: FoldAndCommit with its folded polynomial kept on the device
            off_b, lens_b = sum(lens[:pack_sizes[0]]), lens[pack_sizes[0]:pack_sizes[0] + pack_sizes[1]]
            d_fold = torch.full((len(case["folds"][1]) * c.fr_limbs,), -1, dtype=torch.int64, device="cuda")
            digest = gm.fflonk.fold_commit_device(d.data_ptr() + 8 * off_b * c.fr_limbs, lens_b, rb, d_fold.data_ptr(), s.cuda_stream)
        s.synchronize()
        hc, hf, hw, hW = gm.fflonk.OpenW(packs, points, case["gamma"], rb)
        hWP = gm.fflonk.OpenWPrime(packs, points, hf, case["gamma"], hw, case["z"], rb)
        assert all((a == b).all() for a, b in zip(claimed, hc)) and all((a == b).all() for a, b in zip(folded_claimed, hf))
        assert (W == hW).all() and (WP == hWP).all()
        assert (d_w.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == hw).all()
        assert (d_fold.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == mont(c, case["folds"][1])).all()
        assert (digest == gm.fflonk.FoldAndCommit(packs[1], rb)).all()
        assert (d.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == flat).all()  # inputs unchanged
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_refusals(gm, curve):
    c = gm.CURVES[curve]
    rng = rng_for(0xFF24, CURVES.index(curve))
    g, pts = _bases(gm, curve, 200)
    rb = g.register_bases(points=pts)
    g2 = gm.G2Affine(curve)
    rb2 = g2.register_bases(points=g2.generate_points(64, 0x5EED, 0xA11))
    el = lambda n: random_field_limbs(rng, c.r, c.fr_limbs, n)
    f, s, gamma, z = el(10), el(2), el(1)[0], el(1)[0]
    one, zero, minus_one = mont(c, [1]), mont(c, [0]), mont(c, [c.r - 1])
    omega3 = mont(c, [fm.ith_root_one(3, c.r, c.fr_mult_gen)])

    def both(packs, points, bases, text):
        ts = [fm.next_divisor(len(p), c.r) or 0 if len(p) else 0 for p in packs]
        wlen = max([t * max(q.shape[0] for q in p) for t, p in zip(ts, packs) if len(p)], default=0)
        folded = [np.zeros((t * np.asarray(q).reshape(-1, c.fr_limbs).shape[0], c.fr_limbs), dtype=np.uint64) for t, q in zip(ts, points)]
        with pytest.raises(ValueError) as e:
            gm.fflonk.OpenW(packs, points, gamma, bases)
        assert text in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            gm.fflonk.OpenWPrime(packs, points, folded, gamma, np.zeros((wlen, c.fr_limbs), dtype=np.uint64), z, bases)
        assert text in str(e.value), str(e.value)
    try:
        both([], [], rb, "no pack of polynomials")
        both([[f]], [s], rb2, "fflonk commits and opens over G1 bases only")

        class Unknown:
            handle, group = 1 << 40, g
        both([[f]], [s], Unknown(), "unknown bases handle")
        both([[f], []], [s, s], rb, "pack 1 holds no polynomial")
        both([[f], [f]], [s, s[:0]], rb, "pack 1 has no opening point")
        both([[f], [f[:0], f[:0]]], [s, s], rb, "polynomial 1 is empty")
        gm.fflonk.OpenW([[f, f[:0]]], [s], gamma, rb)  # an empty member of a non-empty pack is the zero polynomial
        # two equal points in an extended set: z_a^t = z_b^t, and z = 0 with t > 1
        both([[f], [f, f]], [s, np.concatenate([one, minus_one])], rb, "set 1 holds the same point twice (points 0 and 3)")
        both([[f, f, f]], [np.stack([s[0], ints_mul(c, s[0], omega3)])], rb, "set 0 holds the same point twice (points 0 and 5)")
        both([[f, f]], [zero], rb, "set 0 holds the same point twice (points 0 and 1)")
        both([[f]], [np.stack([s[0], s[0]])], rb, "set 0 holds the same point twice (points 0 and 1)")
        claimed, folded, w1, _ = gm.fflonk.OpenW([[f], [f, f]], [zero, one], gamma, rb)  # z = 0 with t = 1; 1 next to it in another pack
        gm.fflonk.OpenWPrime([[f], [f, f]], [zero, one], folded, gamma, w1, z, rb)
        with pytest.raises(ValueError, match="the number of packs of polynomials should be the same as the number of pack of points"):
            gm.fflonk.OpenW([[f], [f]], [s], gamma, rb)
        n = next(n for n in itertools.count(1 << 20) if all((c.r - 1) % t for t in range(n, n + 101)))
        with pytest.raises(ValueError, match="did not find any divisor of r-1"):
            gm.fflonk.NextDivisor(curve, n)
        for bases, text in ((rb2, "fflonk commits and opens over G1 bases only"), (Unknown(), "unknown bases handle")):
            with pytest.raises(ValueError) as e:
                gm.fflonk.FoldAndCommit([f], bases)
            assert text in str(e.value)
        with pytest.raises(ValueError) as e:
            gm.fflonk.FoldAndCommit([el(101), el(3)], rb)  # 2 * 101 > 200 registered points
        assert str(e.value) == ERR_SIZE
        gm.fflonk.FoldAndCommit([el(100), el(3)], rb)
        assert not gm.fflonk.FoldAndCommit([np.zeros_like(f), f[:0]], rb).any()  # an all-zero fold commits to infinity
        L = gm._lib.load()  # pointer pairs: neither / both
        import ctypes
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        lens, sizes, npts = (ctypes.c_size_t * 1)(10), (ctypes.c_size_t * 1)(1), (ctypes.c_size_t * 1)(2)
        out, out2, jac, w = np.zeros_like(s), np.zeros_like(s), np.zeros(g.jac_limbs, dtype=np.uint64), np.zeros_like(f)
        assert L.gmsm_fflonk_open_w(rb.handle, P(f), None, lens, sizes, 1, P(s), npts, P(gamma), None, P(out), P(out2), None, None,
                                    P(jac)) == gm._lib.GMSM_ERR_ARG
        assert "exactly one of out_w (host) / d_out_w (device)" in gm._lib.last_error()
        assert L.gmsm_fflonk_open_wprime(rb.handle, P(f), None, lens, sizes, 1, P(s), npts, P(out), P(gamma), P(w), P(w), P(z), None,
                                         P(jac)) == gm._lib.GMSM_ERR_ARG
        assert "exactly one of w (host) / d_w (device)" in gm._lib.last_error()
    finally:
        rb.release()
        rb2.release()


def ints_mul(c, a, b):
    """the product of two field elements given as Montgomery limbs, as Montgomery limbs"""
    return mont(c, [true(c, a)[0] * true(c, b)[0]])[0]


@pytest.mark.parametrize("curve", CURVES)
def test_size_condition_at_its_edge(gm, curve):
    """shplonk commits wPrime over maxSizePolys + sum t_i m_i - 1 coefficients of the FOLDED sizes: a key one point short is
    refused by both entries, a key of exactly that size serves them"""
    c = gm.CURVES[curve]
    rng = rng_for(0xFF25, CURVES.index(curve))
    el = lambda n: random_field_limbs(rng, c.r, c.fr_limbs, n)
    gamma, z = el(1)[0], el(1)[0]
    # maxSizePolys from the longest folded polynomial (3 * 40), and from the largest extended set (6 * 2 + 1 > every folded length)
    for pack_lens, sizes in ((((40, 7, 1), (5,)), (2, 3)), (((2, 1, 1, 0, 2), (3,)), (2, 1))):
        packs, points = [[el(n) for n in lens] for lens in pack_lens], [el(m) for m in sizes]
        ts = [fm.next_divisor(len(p), c.r) for p in pack_lens]
        need = max(max(t * max(lens) for t, lens in zip(ts, pack_lens)), max(t * m for t, m in zip(ts, sizes)) + 1) + \
            sum(t * m for t, m in zip(ts, sizes)) - 1
        g, pts = _bases(gm, curve, need)
        short, exact = g.register_bases(points=pts[:need - 1]), g.register_bases(points=pts)
        try:
            wlen = max(t * max(lens) for t, lens in zip(ts, pack_lens))
            w = np.zeros((wlen, c.fr_limbs), dtype=np.uint64)
            folded = [np.zeros((t * m, c.fr_limbs), dtype=np.uint64) for t, m in zip(ts, sizes)]
            with pytest.raises(ValueError) as e:
                gm.fflonk.OpenW(packs, points, gamma, short)
            assert str(e.value) == ERR_SIZE
            with pytest.raises(ValueError) as e:
                gm.fflonk.OpenWPrime(packs, points, folded, gamma, w, z, short)
            assert str(e.value) == ERR_SIZE
            claimed, folded, w, W = gm.fflonk.OpenW(packs, points, gamma, exact)
            gm.fflonk.OpenWPrime(packs, points, folded, gamma, w, z, exact)
            tr = lambda a: true(c, a)
            mw, mclaimed, mfolded, _ = fm.reference_batch_open([[tr(p) for p in pack] for pack in packs], [tr(s) for s in points],
                                                               tr(gamma)[0], tr(z)[0], c.r, c.fr_mult_gen)
            assert [[tr(row) for row in v] for v in claimed] == mclaimed and [tr(v) for v in folded] == mfolded
            assert [x for x in tr(w)] == (mw + [0] * wlen)[:wlen]
        finally:
            short.release()
            exact.release()
