"""The mpcsetup point updates on the device (gmsm_scale.h through include/gmsm.h and gnark-crypto_amd/mpcsetup.py), all six
groups.

Every group is cyclic of prime order r, so for inputs A[i] = [k_i]Gen the expected outputs are [k_i s_i mod r]Gen - Python
integers followed by the separately tested fixed-base BatchScalarMultiplication(Gen, .) - compared limb for limb:
  - per-point scalars for sizes around the wave and block sizes, inputs at infinity, the scalars 0, 1, 2, r - 1, both sides
    of 2^GLV_BITS and a single-limb value; the input is not modified
  - one scalar for all (0, 1, r - 1, random): equals the per-point call with the scalar repeated, and the closed form
  - UpdateMonomials: out[0] = A[0], equals the batch with host-made powers, and the ceremony identity - [Gen] * n updated
    by r1, r2, r3 is NewSRS with tau = r1 r2 r3
  - 64 points per group against the oracle's own scalar multiplication on the host (independent of the fixed-base kernel)
  - linearCombinations for several segmentations on each side of the fused small-n MultiExp's limit, members at infinity,
    and shifted = [tau] truncated for a geometric slice
  - device pointers made on a torch stream give the same bits, the output may alias the input, inputs are not modified
  - four threads updating at once"""
import threading

import numpy as np
import pytest

from conftest import ALL_GROUPS, random_field_limbs, rng_for, scalars_from_ints

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000]
SIZES_WIDE = [1, 3, 64, 65, 257]  # BW6-761 and the G2 groups
IDS = [f"{c}-{w}" for c, w in ALL_GROUPS]


def sizes_of(curve, which):
    return SIZES if which == "g1" and curve != "bw6_761" else SIZES_WIDE


def from_limbs(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    raw, w = a.tobytes(), 8 * a.shape[-1]
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def group_of(gm, curve, which):
    return (gm.G1Affine if which == "g1" else gm.G2Affine)(curve)


def points_of(gm, curve, which, vals):
    """[v]Gen for python ints v"""
    g = group_of(gm, curve, which)
    return g.BatchScalarMultiplication(g.generator, scalars_from_ints(gm.CURVES[curve], vals))


def mirror(gm, which, name):
    return getattr(gm.mpcsetup, name + ("G1" if which == "g1" else "G2"))


def random_ints(rng, c, n):
    return from_limbs(random_field_limbs(rng, c.r, c.fr_limbs, n))


def special_scalars(gm, c):
    bits = gm.curves.GlvParams(c).bits
    return [0, 1, 2, c.r - 1, (1 << bits) - 1, 1 << bits, 0xDEADBEEF12345]


_cache = {}


def case_of(gm, curve, which):
    """k (every 7th 0), s (every 5th special, from index 2 so that they meet finite points), A = [k]Gen, expected [k s]Gen for the largest size of the group - made once"""
    key = (curve, which)
    if key not in _cache:
        c = gm.CURVES[curve]
        n = max(sizes_of(curve, which))
        rng = rng_for(0x3C0, ALL_GROUPS.index(key))
        k, s = random_ints(rng, c, n), random_ints(rng, c, n)
        sp = special_scalars(gm, c)
        for i in range(0, n, 7):
            k[i] = 0
        for j, i in enumerate(range(2, n, 5)):
            s[i] = sp[j % len(sp)]
        pts = points_of(gm, curve, which, k)
        exp = points_of(gm, curve, which, [a * b % c.r for a, b in zip(k, s)])
        for a in (pts, exp):
            a.setflags(write=False)
        _cache[key] = (k, s, pts, exp)
    return _cache[key]


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_per_point_scalars(gm, curve, which):
    c = gm.CURVES[curve]
    k, s, pts, exp = case_of(gm, curve, which)
    sc = scalars_from_ints(c, s)
    for n in sizes_of(curve, which):
        a = pts[:n].copy()
        got = mirror(gm, which, "BatchScale")(curve, a, sc[:n])
        assert (a == pts[:n]).all()
        assert (got == exp[:n]).all(), (curve, which, n, np.nonzero((got != exp[:n]).any(axis=1))[0][:8])
    assert not exp[0].any() and (len(exp) < 3 or (pts[2].any() and not exp[2].any()))  # infinity in; scalar 0 on a finite point


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_one_scalar_for_all(gm, curve, which):
    c = gm.CURVES[curve]
    k, _, pts, _ = case_of(gm, curve, which)
    nmax = len(k)
    rnd = random_ints(rng_for(0x3C1, ALL_GROUPS.index((curve, which))), c, 1)[0]
    for s in (0, 1, c.r - 1, rnd):
        one = scalars_from_ints(c, [s])
        exp = points_of(gm, curve, which, [a * s % c.r for a in k])
        for n in sizes_of(curve, which):
            got = mirror(gm, which, "Scale")(curve, pts[:n], one)
            assert (got == mirror(gm, which, "BatchScale")(curve, pts[:n], np.tile(one, (n, 1)))).all(), (curve, which, n, s)
            assert (got == exp[:n]).all(), (curve, which, n, s)
        if s == 0:
            assert not exp.any()
        if s == 1:
            assert (exp == pts[:nmax]).all()


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_update_monomials(gm, curve, which):
    c = gm.CURVES[curve]
    rng = rng_for(0x3C2, ALL_GROUPS.index((curve, which)))
    nmax = 1000
    k = random_ints(rng, c, nmax)
    for i in range(3, nmax, 7):
        k[i] = 0
    pts = points_of(gm, curve, which, k)
    for r in (0, 1, random_ints(rng, c, 1)[0]):
        powers = [pow(r, i, c.r) for i in range(nmax)]
        exp = points_of(gm, curve, which, [a * p % c.r for a, p in zip(k, powers)])
        rl = scalars_from_ints(c, [r])
        for n in (2, 3, 64, 65, 1000):
            got = mirror(gm, which, "UpdateMonomials")(curve, pts[:n], rl)
            assert (got[0] == pts[0]).all()
            assert (got == mirror(gm, which, "BatchScale")(curve, pts[:n], scalars_from_ints(c, powers[:n]))).all(), (curve, which, n, r)
            assert (got == exp[:n]).all(), (curve, which, n, r)


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_ceremony_identity(gm, curve, which):
    """InitializeSetup, three contributions, and the result is NewSRS with tau = r1 r2 r3"""
    c = gm.CURVES[curve]
    g = group_of(gm, curve, which)
    n = 65
    r1, r2, r3 = random_ints(rng_for(0x3C3, ALL_GROUPS.index((curve, which))), c, 3)
    a = np.tile(g.generator, (n, 1))
    for r in (r1, r2, r3):
        a = mirror(gm, which, "UpdateMonomials")(curve, a, scalars_from_ints(c, [r]))
    tau = r1 * r2 * r3 % c.r
    assert (a == points_of(gm, curve, which, [pow(tau, i, c.r) for i in range(n)])).all()


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_against_the_oracle(gm, oracle_mod, curve, which):
    c = gm.CURVES[curve]
    o = oracle_mod.Oracle(curve, which)
    rng = rng_for(0x3C4, ALL_GROUPS.index((curve, which)))
    n = 64
    g = group_of(gm, curve, which)
    pts = g.generate_points(n, 0xABCDEF, 0x1234567)
    pts[9] = 0
    s = random_ints(rng, c, n)
    sp = special_scalars(gm, c)
    s[:len(sp)] = sp
    got = mirror(gm, which, "BatchScale")(curve, pts, scalars_from_ints(c, s))
    for i in range(n):
        exp = o.jac_to_affine(o.scalar_mul(pts[i], s[i])) if pts[i].any() and s[i] else np.zeros_like(pts[i])
        assert (got[i] == exp).all(), (curve, which, i)


def fused_limit(g):
    """the largest n a MultiExp over bases taken anew runs in the fused small-n kernel"""
    lo, hi = 1, 1 << 20
    assert g.default_plan(lo)["fused"] and not g.default_plan(hi)["fused"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if g.default_plan(mid)["fused"] else (lo, mid)
    return lo


def expected_combinations(c, k, r, ends):
    last = {e - 1 for e in ends}
    t = sum(pow(r, i, c.r) * k[i] for i in range(len(k)) if i not in last) % c.r
    s = sum(pow(r, i, c.r) * k[i + 1] for i in range(len(k)) if i not in last) % c.r
    return t, s


@pytest.mark.parametrize("curve,which", ALL_GROUPS, ids=IDS)
def test_linear_combinations(gm, curve, which):
    c = gm.CURVES[curve]
    g = group_of(gm, curve, which)
    rng = rng_for(0x3C5, ALL_GROUPS.index((curve, which)))
    small = 12
    ns = [small]
    if which == "g1" and curve != "bw6_761":
        limit = fused_limit(g)
        ns += [limit, limit + 2]  # both MultiExps (n and n - 1 points) fused / both in the sorted pipeline
    r = random_ints(rng, c, 1)[0]
    rl = scalars_from_ints(c, [r])
    k = random_ints(rng, c, max(ns))
    for i in range(1, len(k), 7):
        k[i] = 0  # members at infinity
    pts = points_of(gm, curve, which, k)
    for n in ns:
        cases = [[n], list(range(2, n + 1, 2))] if n > small else [[2], [n], [3, 5, 9], list(range(2, n + 1, 2))]
        for ends in cases:
            m = ends[-1]
            t, s = mirror(gm, which, "linearCombinations")(curve, pts[:m], rl, ends)
            et, es = expected_combinations(c, k[:m], r, ends)
            exp = points_of(gm, curve, which, [et, es])
            assert (g.jac_to_affine(t) == exp[0]).all(), (curve, which, n, ends[:4])
            assert (g.jac_to_affine(s) == exp[1]).all(), (curve, which, n, ends[:4])
    # a geometric slice A[i] = [tau^i]Gen: shifted = [tau] truncated
    tau = random_ints(rng, c, 1)[0]
    geo = points_of(gm, curve, which, [pow(tau, i, c.r) for i in range(small)])
    t, s = mirror(gm, which, "linearCombinations")(curve, geo, rl, [small])
    t_aff = g.jac_to_affine(t).reshape(1, -1)
    assert (g.jac_to_affine(s) == mirror(gm, which, "Scale")(curve, t_aff, scalars_from_ints(c, [tau]))[0]).all()


@pytest.mark.parametrize("which", ["g1", "g2"])
def test_device_pointers_on_a_torch_stream(gm, which):
    import torch
    curve = "bn254"
    c = gm.CURVES[curve]
    rng = rng_for(0x3C6, which == "g2")
    n = 300
    k, sv = random_ints(rng, c, n), random_ints(rng, c, n)
    k[4] = 0
    r = random_ints(rng, c, 1)[0]
    rl, sc = scalars_from_ints(c, [r]), scalars_from_ints(c, sv)
    pts = points_of(gm, curve, which, k)
    exp_scale = mirror(gm, which, "BatchScale")(curve, pts, sc)
    exp_one = mirror(gm, which, "Scale")(curve, pts, sc[:1])
    exp_upd = mirror(gm, which, "UpdateMonomials")(curve, pts, rl)
    exp_t, exp_s = mirror(gm, which, "linearCombinations")(curve, pts, rl, [100, 300])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = torch.from_numpy(pts.view(np.int64).copy()).cuda() * 1  # produced by a kernel on st
        dsc = torch.from_numpy(sc.view(np.int64).copy()).cuda() * 1
        out, one, upd = torch.empty_like(d), torch.empty_like(d), torch.empty_like(d)
        gm.mpcsetup.batch_scale_device(curve, which, d.data_ptr(), n, dsc.data_ptr(), n, out.data_ptr(), st.cuda_stream)
        gm.mpcsetup.batch_scale_device(curve, which, d.data_ptr(), n, dsc.data_ptr(), 1, one.data_ptr(), st.cuda_stream)
        gm.mpcsetup.update_monomials_device(curve, which, d.data_ptr(), n, rl, upd.data_ptr(), st.cuda_stream)
        t, s = gm.mpcsetup.linear_combinations_device(curve, which, d.data_ptr(), n, rl, [100, 300], st.cuda_stream)
        in1, in2 = d * 1, d * 1
        gm.mpcsetup.batch_scale_device(curve, which, in1.data_ptr(), n, dsc.data_ptr(), n, in1.data_ptr(), st.cuda_stream)  # aliased
        gm.mpcsetup.update_monomials_device(curve, which, in2.data_ptr(), n, rl, in2.data_ptr(), st.cuda_stream)
    st.synchronize()
    host = lambda x: x.cpu().numpy().view(np.uint64).reshape(pts.shape)
    assert (host(out) == exp_scale).all() and (host(one) == exp_one).all() and (host(upd) == exp_upd).all()
    assert (host(in1) == exp_scale).all() and (host(in2) == exp_upd).all()
    g = group_of(gm, curve, which)
    assert (g.jac_to_affine(t) == g.jac_to_affine(exp_t)).all() and (g.jac_to_affine(s) == g.jac_to_affine(exp_s)).all()
    assert (host(d) == pts).all()  # the input of the non-aliased calls


def test_four_threads_at_once(gm):
    c = gm.CURVES["bn254"]
    rng = rng_for(0x3C7)
    inputs = [points_of(gm, "bn254", "g1", random_ints(rng, c, 2048)) for _ in range(4)]
    rs = [scalars_from_ints(c, random_ints(rng, c, 1)) for _ in range(4)]
    exp = [gm.mpcsetup.UpdateMonomialsG1("bn254", p, r) for p, r in zip(inputs, rs)]
    errs = []

    def run(i):
        try:
            for _ in range(3):
                assert (gm.mpcsetup.UpdateMonomialsG1("bn254", inputs[i], rs[i]) == exp[i]).all()
        except Exception as e:  # noqa: BLE001  (reported below)
            errs.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
