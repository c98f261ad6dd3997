"""KZG opening on the device (gmsm_poly.h through include/gmsm.h and gnark-crypto_amd/kzg.py), every curve's G1:
  - DividePolyByXMinusA / PolyEval equal a Python big-int model of eval + dividePolyByXminusA (kzg.go:55-63, :565-583)
    limb for limb, from one coefficient up to 2^20 and around the kernels' lane and tile boundaries
  - Open's H equals ResidentBases.MultiExp of the model's quotient, over plain bases and over window tables
  - over an SRS [tau^i]G built by BatchScalarMultiplication, H = [h(tau)]G (the CPU oracle's) and h(tau)(tau - a) + f(a) = f(tau)
  - BatchOpenSinglePoint equals fold-then-divide in the model, for unequal lengths with a member of length 1
  - device-pointer inputs made on a torch stream give the same bits; inputs are never modified
  - the reference's size errors; four threads opening on one handle at once"""
import threading

import numpy as np
import pytest

from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
# lengths: tiny, one lane / one tile of the kernels (2048 coefficients below 2^14) +- 1, two tiles + 1, the 2^16 and 2^20 shapes
SIZES = [1, 2, 3, 31, 32, 33, 2047, 2048, 2049, 4097, (1 << 16) + 1, 1 << 20]


def ints(a):
    """rows of uint64 limbs -> python ints (the Montgomery representatives)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    raw = a.reshape(-1, a.shape[-1]).astype("<u8").tobytes()
    w = 8 * a.shape[-1]
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def limbs(vals, nl):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(nl)] for v in vals], dtype=np.uint64).reshape(-1, nl)


def model(f, a_true, r):
    """(h, f(a)) on Montgomery representatives: y_i = f_i + a y_(i+1) is linear, so it holds for x R as for x"""
    y = 0
    ys = [0] * len(f)
    for i in range(len(f) - 1, -1, -1):
        y = (f[i] + a_true * y) % r
        ys[i] = y
    return ys[1:], ys[0]


def points_for(c, rng):
    """point limbs (Montgomery) for 0, 1, r - 1 and a random element, with their true values"""
    R = c.fr_R
    out = []
    for v in (0, 1, c.r - 1, int(ints(random_field_limbs(rng, c.r, c.fr_limbs, 1))[0]) * pow(R, -1, c.r) % c.r):
        out.append((limbs([v * R % c.r], c.fr_limbs)[0], v))
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_divide_and_eval_match_model(gm, curve):
    c = gm.CURVES[curve]
    rng = rng_for(0x4B5A, CURVES.index(curve))
    pts = points_for(c, rng)
    polys = []
    for n in SIZES:
        f = random_field_limbs(rng, c.r, c.fr_limbs, n)
        before = f.copy()
        fi = ints(f)
        for pl, pv in (pts if n <= (1 << 16) + 1 else pts[2:]):
            h, val = gm.kzg.DividePolyByXMinusA(curve, f, pl)
            mh, mv = model(fi, pv, c.r)
            assert ints(val) == [mv], (n, pv)
            assert h.shape == (n - 1, c.fr_limbs) and ints(h) == mh, (n, pv)
        assert (f == before).all()
        polys.append(f)
    pl, pv = pts[3]
    vals = gm.kzg.PolyEval(curve, polys, pl)
    assert ints(vals) == [model(ints(f), pv, c.r)[1] for f in polys]


def _bases(gm, curve, n):
    g = gm.G1Affine(curve)
    return g, g.generate_points(n, 0x5EED, 0xA11)


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_open_commits_the_model_quotient(gm, curve, tables):
    c = gm.CURVES[curve]
    rng = rng_for(0x4B5B, CURVES.index(curve), int(tables))
    g, pts = _bases(gm, curve, 5000)
    rb = g.register_bases(points=pts)
    try:
        if tables:
            rb.precompute(0)
        pl, pv = points_for(c, rng)[3]
        for n in (2, 33, 4097, 5000):
            f = random_field_limbs(rng, c.r, c.fr_limbs, n)
            before = f.copy()
            with gm.options(tables=2) if tables else _null():
                claimed, H = gm.kzg.Open(f, pl, rb)
                mh, mv = model(ints(f), pv, c.r)
                jac, err = rb.MultiExp(limbs(mh, c.fr_limbs))
            assert err is None
            assert ints(claimed) == [mv], n
            assert (H == g.jac_to_affine(jac)).all(), n
            assert (f == before).all()
    finally:
        rb.release()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize("curve", CURVES)
def test_open_over_known_tau(gm, oracle_mod, curve):
    """independent of the model: H = [h(tau)]G over the SRS [tau^i]G, and h(tau)(tau - a) + f(a) = f(tau)"""
    c = gm.CURVES[curve]
    rng = rng_for(0x4B5C, CURVES.index(curve))
    R, r = c.fr_R, c.r
    tau = int(ints(random_field_limbs(rng, r, c.fr_limbs, 1))[0])
    n = 3000
    g = gm.G1Affine(curve)
    gen = np.array(g.generate_points(1, 0xC0FFEE, 0xBEEF)[0], dtype=np.uint64)  # a fixed point of G1 as the SRS base
    srs = g.BatchScalarMultiplication(gen, limbs([pow(tau, i, r) * R % r for i in range(n)], c.fr_limbs))
    rb = g.register_bases(points=srs)
    try:
        f = random_field_limbs(rng, r, c.fr_limbs, n)
        a = int(ints(random_field_limbs(rng, r, c.fr_limbs, 1))[0])
        claimed, H = gm.kzg.Open(f, limbs([a * R % r], c.fr_limbs)[0], rb)
        h, _ = gm.kzg.DividePolyByXMinusA(curve, f, limbs([a * R % r], c.fr_limbs)[0])
        Rinv = pow(R, -1, r)
        hv = [x * Rinv % r for x in ints(h)]
        fv = [x * Rinv % r for x in ints(f)]
        h_tau = sum(x * pow(tau, i, r) for i, x in enumerate(hv)) % r
        f_tau = sum(x * pow(tau, i, r) for i, x in enumerate(fv)) % r
        fa = ints(claimed)[0] * Rinv % r
        assert (h_tau * (tau - a) + fa) % r == f_tau
        o = oracle_mod.Oracle(curve, "g1")
        exp = o.msm_affine(gen.reshape(1, -1), limbs([h_tau * R % r], c.fr_limbs), nthreads=1)
        assert (H == np.asarray(exp).reshape(H.shape)).all()
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_batch_open_matches_fold_then_divide(gm, curve):
    c = gm.CURVES[curve]
    rng = rng_for(0x4B5D, CURVES.index(curve))
    g, pts = _bases(gm, curve, 3000)
    rb = g.register_bases(points=pts)
    try:
        pl, pv = points_for(c, rng)[3]
        gl, gv = points_for(c, rng)[3]
        for lens in ((40,), (1, 2500), (17, 1, 3000, 5, 2048, 2049, 300)):
            polys = [random_field_limbs(rng, c.r, c.fr_limbs, n) for n in lens]
            before = [p.copy() for p in polys]
            values, H = gm.kzg.BatchOpenSinglePoint(polys, pl, gl, rb)
            assert ints(values) == [model(ints(p), pv, c.r)[1] for p in polys]
            maxlen = max(lens)
            F = [0] * maxlen
            for p in reversed(polys):  # sum_i gamma^i f_i (Horner in gamma, on Montgomery representatives: gamma's true value)
                pi = ints(p)
                F = [(F[j] * gv + (pi[j] if j < len(pi) else 0)) % c.r for j in range(maxlen)]
            mh, _ = model(F, pv, c.r)
            jac, err = rb.MultiExp(limbs(mh, c.fr_limbs))
            assert err is None and (H == g.jac_to_affine(jac)).all(), lens
            assert all((p == b).all() for p, b in zip(polys, before))
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointers_on_a_torch_stream(gm, curve):
    import torch
    c = gm.CURVES[curve]
    rng = rng_for(0x4B5E, CURVES.index(curve))
    g, pts = _bases(gm, curve, 5000)
    rb = g.register_bases(points=pts)
    try:
        pl, _ = points_for(c, rng)[3]
        gl, _ = points_for(c, rng)[3]
        lens = [4097, 1, 300]
        polys = [random_field_limbs(rng, c.r, c.fr_limbs, n) for n in lens]
        flat = np.concatenate(polys)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            src = torch.from_numpy(flat.view(np.int64).copy()).cuda(non_blocking=False)
            d = src * 1  # produced by a kernel on s
            stream = s.cuda_stream
            claimed, H = gm.kzg.open_device(d.data_ptr(), lens[0], pl, rb, stream)
            out_h = torch.empty((lens[0] - 1) * c.fr_limbs, dtype=torch.int64, device="cuda")
            val = gm.kzg.divide_device(curve, d.data_ptr(), lens[0], pl, out_h.data_ptr(), stream)
            values, BH = gm.kzg.batch_open_device(d.data_ptr(), lens, pl, gl, rb, stream)
            evals = gm.kzg.poly_eval_device(curve, d.data_ptr(), lens, pl, stream)
        s.synchronize()
        hc, vc = gm.kzg.Open(polys[0], pl, rb)
        assert (claimed == hc).all() and (H == vc).all()
        h_host, v_host = gm.kzg.DividePolyByXMinusA(curve, polys[0], pl)
        assert (val == v_host).all()
        assert (out_h.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == h_host).all()
        bv, bh = gm.kzg.BatchOpenSinglePoint(polys, pl, gl, rb)
        assert (values == bv).all() and (BH == bh).all() and (evals == bv).all()
        assert (d.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs) == flat).all()  # inputs unchanged
    finally:
        rb.release()


@pytest.mark.parametrize("curve", CURVES)
def test_reference_size_errors(gm, curve):
    c = gm.CURVES[curve]
    g, pts = _bases(gm, curve, 64)
    rb = g.register_bases(points=pts)
    msg = "invalid polynomial size (larger than SRS or == 0)"
    zero = np.zeros(c.fr_limbs, dtype=np.uint64)
    try:
        for n in (0, 1, 65):
            with pytest.raises(ValueError, match=r"invalid polynomial size \(larger than SRS or == 0\)"):
                gm.kzg.Open(np.ones((n, c.fr_limbs), dtype=np.uint64), zero, rb)
        for lens in ((1,), (1, 1), (64, 65), (3, 0)):
            with pytest.raises(ValueError) as e:
                gm.kzg.BatchOpenSinglePoint([np.ones((n, c.fr_limbs), dtype=np.uint64) for n in lens], zero, zero, rb)
            assert str(e.value) == msg, lens
        h, v = gm.kzg.DividePolyByXMinusA(curve, np.ones((1, c.fr_limbs), dtype=np.uint64), zero)  # n == 1: f(a), empty h
        assert h.shape == (0, c.fr_limbs) and (v == 1).all()
    finally:
        rb.release()


def test_concurrent_opens_on_one_handle(gm):
    curve = "bn254"
    c = gm.CURVES[curve]
    rng = rng_for(0x4B5F)
    g, pts = _bases(gm, curve, 1 << 14)
    rb = g.register_bases(points=pts)
    try:
        pl, _ = points_for(c, rng)[3]
        polys = [random_field_limbs(rng, c.r, c.fr_limbs, n) for n in (1 << 14, 5000, 33, 9000)]
        seq = [gm.kzg.Open(p, pl, rb) for p in polys]
        got = [None] * 4
        errs = []

        def run(i):
            try:
                for _ in range(3):
                    got[i] = gm.kzg.Open(polys[i], pl, rb)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs
        for (sc, sh), (gc, gh) in zip(seq, got):
            assert (sc == gc).all() and (sh == gh).all()
    finally:
        rb.release()
