"""GPU parity tests: every stage of the HIP pipeline, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Bit-exact: integer work, the bar is equality of limbs (affine X,Y Montgomery limbs for MSM results).
Run with `pytest -m gpu` on an MI355X."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ALL_GROUPS, int_to_limbs, random_field_limbs, random_scalars, rng_for, scalars_from_ints

pytestmark = pytest.mark.gpu

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _group(gm, curve, which):
    return (gm.G1Affine if which == "g1" else gm.G2Affine)(curve)


def _edge_values(modulus, nlimbs, R):
    vals = [0, 1, 2, modulus - 1, modulus - 2, R % modulus, R * R % modulus, (1 << 64) - 1, 1 << 64, (1 << (64 * (nlimbs - 1))) - 1,
            modulus >> 1, (modulus >> 1) + 1]
    return np.array([int_to_limbs(v % modulus, nlimbs) for v in vals], dtype=np.uint64)


# ------------------------------------------------------------------ field kernels
@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_field_ops_match_oracle(gm, oracle_mod, curve, which):
    L = gm._lib.load()
    g = _group(gm, curve, which)
    c = g.curve
    rng = rng_for(1, g.gid)
    fields = [(0, f"{c.name}_fp", c.p, c.fp_limbs, c.fp_R), (1, f"{c.name}_fr", c.r, c.fr_limbs, c.fr_R)]
    for fid, name, mod, nl, R in fields:
        F = oracle_mod.Field(name, nl)
        a = np.concatenate([_edge_values(mod, nl, R), random_field_limbs(rng, mod, nl, 500)])
        b = np.concatenate([random_field_limbs(rng, mod, nl, 500), _edge_values(mod, nl, R)])
        # all pairs of edge values too
        e = _edge_values(mod, nl, R)
        a = np.concatenate([a, np.repeat(e, len(e), axis=0)])
        b = np.concatenate([b, np.tile(e, (len(e), 1))])
        for op, fn in [(0, F.mul), (1, F.add), (2, F.sub)]:
            out = np.zeros_like(a)
            assert L.gmsm_debug_field_op(g.gid, fid, op, P(a), P(b), len(a), P(out)) == 0, gm._lib.last_error()
            exp = np.array([fn(x, y) for x, y in zip(a, b)])
            assert (out == exp).all(), (name, op)
        for op, fn in [(3, F.neg), (4, F.dbl), (5, F.sqr), (6, F.from_mont)]:
            out = np.zeros_like(a)
            assert L.gmsm_debug_field_op(g.gid, fid, op, P(a), None, len(a), P(out)) == 0, gm._lib.last_error()
            exp = np.array([fn(x) for x in a])
            assert (out == exp).all(), (name, op)
    # the coordinate field through the lazy-limb code of the pipeline (field id 3)
    if g.coord_limbs == c.fp_limbs:
        F = oracle_mod.Field(f"{c.name}_fp", c.fp_limbs)
        e = _edge_values(c.p, c.fp_limbs, c.fp_R)
        a = np.concatenate([np.repeat(e, len(e), axis=0), random_field_limbs(rng, c.p, c.fp_limbs, 400)])
        b = np.concatenate([np.tile(e, (len(e), 1)), random_field_limbs(rng, c.p, c.fp_limbs, 400)])
    else:
        F = oracle_mod.Field(f"{c.name}_e2", 2 * c.fp_limbs)
        e1 = _edge_values(c.p, c.fp_limbs, c.fp_R)
        e = np.concatenate([np.concatenate([x, y]) [None, :] for x in e1[:6] for y in e1[:6]])
        a = np.concatenate([np.repeat(e, 6, axis=0)[: 200], random_field_limbs(rng, c.p, c.fp_limbs, 400).reshape(200, -1)])
        b = np.concatenate([np.tile(e, (6, 1))[: 200], random_field_limbs(rng, c.p, c.fp_limbs, 400).reshape(200, -1)])
    for op, fn in [(0, F.mul), (1, F.add), (2, F.sub)]:
        out = np.zeros_like(a)
        assert L.gmsm_debug_field_op(g.gid, 3, op, P(a), P(b), len(a), P(out)) == 0, gm._lib.last_error()
        assert (out == np.array([fn(x, y) for x, y in zip(a, b)])).all(), ("lazy", op)
    for op, fn in [(3, F.neg), (4, F.dbl), (5, F.sqr)]:
        out = np.zeros_like(a)
        assert L.gmsm_debug_field_op(g.gid, 3, op, P(a), None, len(a), P(out)) == 0, gm._lib.last_error()
        assert (out == np.array([fn(x) for x in a])).all(), ("lazy", op)
    if g.coord_limbs != c.fp_limbs:  # Fp2
        F = oracle_mod.Field(f"{c.name}_e2", 2 * c.fp_limbs)
        a = random_field_limbs(rng, c.p, c.fp_limbs, 600).reshape(300, -1)
        b = random_field_limbs(rng, c.p, c.fp_limbs, 600).reshape(300, -1)
        a[0] = 0
        b[1] = 0
        a[2, c.fp_limbs:] = 0
        b[3, : c.fp_limbs] = 0
        for op, fn in [(0, F.mul), (1, F.add), (2, F.sub)]:
            out = np.zeros_like(a)
            assert L.gmsm_debug_field_op(g.gid, 2, op, P(a), P(b), len(a), P(out)) == 0, gm._lib.last_error()
            assert (out == np.array([fn(x, y) for x, y in zip(a, b)])).all(), ("e2", op)
        for op, fn in [(3, F.neg), (4, F.dbl), (5, F.sqr)]:
            out = np.zeros_like(a)
            assert L.gmsm_debug_field_op(g.gid, 2, op, P(a), None, len(a), P(out)) == 0, gm._lib.last_error()
            assert (out == np.array([fn(x) for x in a])).all(), ("e2", op)


# ------------------------------------------------------------------ group law incl. every special case
@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_group_ops_match_oracle(gm, oracle_mod, curve, which):
    L = gm._lib.load()
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 48
    pts = o.gen_points(n, 7, 11)
    other = o.gen_points(n, 1000, 13)
    # accumulators: running sums in XYZZ (non-trivial ZZ/ZZZ)
    accs = []
    acc = o.xyzz_infinity()
    for i in range(n):
        acc = o.xyzz_add_mixed(acc, other[i])
        accs.append(acc.copy())
    accs = np.array(accs)
    # special cases (g1.go:829-854): acc = infinity; point = infinity (0,0); acc == point (doubling); acc == -point
    accs[0] = o.xyzz_infinity()
    pts[1] = 0
    accs[2] = o.xyzz_add_mixed(o.xyzz_infinity(), pts[2])                 # P + P
    accs[3] = o.xyzz_add_mixed(o.xyzz_infinity(), pts[3], negate=True)    # -P + P = inf
    accs[4] = o.xyzz_double(o.xyzz_add_mixed(o.xyzz_infinity(), pts[4]))  # 2P (ZZ != 1) + P
    t = o.xyzz_add_mixed(o.xyzz_infinity(), pts[5]); t = o.xyzz_add_mixed(t, pts[6]); t = o.xyzz_add_mixed(t, pts[6], negate=True)
    accs[5] = t                                                            # (P5 + P6 - P6) has ZZ != 1, equals P5 -> doubling branch
    aff = lambda x: o.jac_to_affine(o.xyzz_to_jac(x))
    for op, neg in [(0, False), (1, True)]:
        out = np.zeros_like(accs)
        assert L.gmsm_debug_group_op(g.gid, op, P(accs), P(pts), n, P(out)) == 0, gm._lib.last_error()
        exp = np.array([o.xyzz_add_mixed(a, p, negate=neg) for a, p in zip(accs, pts)])
        assert (out == exp).all(), ("add_mixed", op, np.nonzero((out != exp).any(axis=1))[0])
        # the lazy-limb group law of the pipeline (ops 4, 5): same formulas, same XYZZ representative
        out2 = np.zeros_like(accs)
        assert L.gmsm_debug_group_op(g.gid, op + 4, P(accs), P(pts), n, P(out2)) == 0, gm._lib.last_error()
        assert all((aff(x) == aff(y)).all() for x, y in zip(out2, exp)), ("lazy add_mixed", op)
        finite = exp[:, 2 * g.coord_limbs: 3 * g.coord_limbs].any(axis=1)  # zz != 0 (infinity may carry any X, Y)
        assert (out2[finite] == exp[finite]).all(), ("lazy add_mixed representative", op)
        assert (out2[~finite][:, 2 * g.coord_limbs:] == 0).all()
    accs2 = np.roll(accs, 7, axis=0).copy()
    accs2[10] = accs[10]           # P + P via full add -> double
    accs2[11] = o.xyzz_infinity()
    out = np.zeros_like(accs)
    assert L.gmsm_debug_group_op(g.gid, 2, P(accs), P(accs2), n, P(out)) == 0, gm._lib.last_error()
    exp = np.array([o.xyzz_add(a, b) for a, b in zip(accs, accs2)])
    assert (out == exp).all(), "xyzz_add"
    out2 = np.zeros_like(accs)
    assert L.gmsm_debug_group_op(g.gid, 6, P(accs), P(accs2), n, P(out2)) == 0, gm._lib.last_error()
    assert all((aff(x) == aff(y)).all() for x, y in zip(out2, exp)), "lazy xyzz_add"
    out = np.zeros_like(accs)
    assert L.gmsm_debug_group_op(g.gid, 3, P(accs), None, n, P(out)) == 0, gm._lib.last_error()
    exp = np.array([o.xyzz_double(a) for a in accs])
    assert (out == exp).all(), "xyzz_double"
    out2 = np.zeros_like(accs)
    assert L.gmsm_debug_group_op(g.gid, 7, P(accs), None, n, P(out2)) == 0, gm._lib.last_error()
    assert all((aff(x) == aff(y)).all() for x, y in zip(out2, exp)), "lazy xyzz_double"


# ------------------------------------------------------------------ scalar decomposition == partitionScalars
@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g1"), ("bw6_761", "g1")])
def test_decompose_matches_partition_scalars(gm, oracle_mod, curve, which):
    L = gm._lib.load()
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    c_ = g.curve
    rng = rng_for(3, g.gid)
    n = 1000
    sc = random_scalars(rng, c_, n)
    edge = scalars_from_ints(c_, [0, 1, 2, c_.r - 1, c_.r - 2, (1 << 16) - 1, 1 << 16, 1 << 15, (1 << 15) - 1, (1 << 64) - 1, 1 << 64,
                                  (1 << 128) + 12345, c_.r >> 1])
    sc[: len(edge)] = edge
    import frontend_cases as fc
    vals = fc.ints_from_mont(c_, sc)
    for c in range(2, 21):  # 8, 9, 10, 12..18, 20: the unrolled kernels of the window table; the rest generic
        nwin = o.nb_chunks(c) if c <= 16 else fc.num_windows(c_.fr_bits, c)
        out = np.zeros((nwin, n), dtype=np.uint32)
        assert L.gmsm_debug_decompose(g.gid, P(sc), n, c, P(out)) == 0, gm._lib.last_error()
        if c <= 16:  # the reference's own digits are 16 bits wide
            exp = o.partition_scalars(sc, c).astype(np.uint32)
        else:        # beyond: the same rule on Python ints (tests/frontend_cases.py, pinned to the reference for c <= 16)
            exp = np.array([[fc.code(d) for d in fc.recode(c_, v, c)] for v in vals], dtype=np.uint32).T
        assert (out == exp).all(), (curve, c)


# ------------------------------------------------------------------ MSM
def _msm_gpu_affine(g, points, scalars):
    aff, err = g.MultiExp(points, scalars)
    assert err is None, err
    return aff


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_msm_sum_of_squares_identity_all_c(gm, oracle_mod, pyref_mod, curve, which):
    """multiexp_test.go:95-126: MSM({i*G},{i*mixer}) for every window size, plus the closed form
    mixer*n(n+1)(2n+1)/6*G (multiexp_test.go:54-60) checked with the independent big-int model."""
    import torch
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    grp = pyref_mod.Group(g.curve, which)
    n = 73
    pts = o.gen_points(n, 1, 1)
    for idx in (5, 17, 40, 66):  # sprinkle infinities (multiexp_test.go:48-52)
        pts[idx] = 0
    mixer = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211122334455667788 % g.curve.r
    sc = scalars_from_ints(g.curve, [(i + 1) * mixer for i in range(n)])
    total = sum((i + 1) ** 2 for i in range(n) if i not in (5, 17, 40, 66)) * mixer % g.curve.r
    expected = grp.mul(total, grp.gen)
    exp_limbs = np.array(grp.point_to_limbs(expected), dtype=np.uint64)
    assert (o.msm_affine(pts, sc, c=7) == exp_limbs).all()
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    for c in range(2, 21):  # 2..16 as the reference does; 17..20 are widths only this engine uses (large n)
        w = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)
        aff = g.jac_to_affine(g.fold_windows(w, c))
        assert (aff == exp_limbs).all(), (curve, which, c)
    assert (_msm_gpu_affine(g, pts, sc) == exp_limbs).all()


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_msm_edge_cases(gm, oracle_mod, curve, which):
    g = _group(gm, curve, which)
    gj = (gm.G1Jac if which == "g1" else gm.G2Jac)(curve)
    o = oracle_mod.Oracle(curve, which)
    c_ = g.curve
    rng = rng_for(5, g.gid)
    # n = 0 -> infinity, no error (Z = 0)
    jac, err = gj.MultiExp(np.zeros((0, g.aff_limbs), dtype=np.uint64), np.zeros((0, g.fr_limbs), dtype=np.uint64))
    assert err is None and (jac[2 * g.coord_limbs:] == 0).all()
    aff, err = g.MultiExp(np.zeros((0, g.aff_limbs), dtype=np.uint64), np.zeros((0, g.fr_limbs), dtype=np.uint64))
    assert err is None and (aff == 0).all()
    # error behaviour (multiexp.go:61-71)
    _, err = g.MultiExp(np.zeros((3, g.aff_limbs), dtype=np.uint64), np.zeros((2, g.fr_limbs), dtype=np.uint64))
    assert err == "len(points) != len(scalars)"
    _, err = g.MultiExp(np.zeros((3, g.aff_limbs), dtype=np.uint64), np.zeros((3, g.fr_limbs), dtype=np.uint64), gm.MultiExpConfig(NbTasks=1025))
    assert err == "invalid config: config.NbTasks > 1024"
    for n in (1, 2, 3, 31, 257):
        pts = o.gen_points(n, 3 + n, 5)
        sc = random_scalars(rng, c_, n)
        assert (_msm_gpu_affine(g, pts, sc) == o.msm_affine(pts, sc)).all(), n
    n = 200
    pts = o.gen_points(n, 99, 7)
    # all-zero scalars -> infinity (multiexp_test.go:164-182)
    assert (_msm_gpu_affine(g, pts, np.zeros((n, g.fr_limbs), dtype=np.uint64)) == 0).all()
    # all-infinity points -> infinity (multiexp_test.go:128-162)
    sc = random_scalars(rng, c_, n)
    assert (_msm_gpu_affine(g, np.zeros_like(pts), sc) == 0).all()
    # special scalars: 1, 2, r-1, powers of two on window boundaries, single-limb values, all equal
    vals = [1, 2, c_.r - 1, 1 << 16, 1 << 32, (1 << 16) - 1, 1 << 15, 12345, (1 << 64) - 1] + [1 << (13 * j) for j in range(1, 12)]
    sc2 = scalars_from_ints(c_, (vals * (n // len(vals) + 1))[:n])
    assert (_msm_gpu_affine(g, pts, sc2) == o.msm_affine(pts, sc2)).all()
    sc3 = np.tile(sc[:1], (n, 1))  # all scalars equal: every window has a single giant bucket
    assert (_msm_gpu_affine(g, pts, sc3) == o.msm_affine(pts, sc3)).all()
    # duplicated (point, scalar) pairs force the doubling branch (multiexp_test.go:241-245); P and -P pairs force P+(-P)
    pts4, sc4 = pts.copy(), sc.copy()
    pts4[100:190] = pts4[10:100]
    sc4[100:190] = sc4[10:100]
    assert (_msm_gpu_affine(g, pts4, sc4) == o.msm_affine(pts4, sc4)).all()
    same = np.tile(pts[:1], (n, 1))  # one base repeated (cf. the 4-point quick SRS, kzg.go:91-115)
    assert (_msm_gpu_affine(g, same, sc) == o.msm_affine(same, sc)).all()
    assert (_msm_gpu_affine(g, same, sc3) == o.msm_affine(same, sc3)).all()


@pytest.mark.parametrize("curve,which,logn", [("bn254", "g1", 14), ("bn254", "g1", 16), ("bn254", "g2", 13),
                                              ("bls12_381", "g1", 13), ("bls12_381", "g2", 12), ("bw6_761", "g1", 12),
                                              ("bw6_761", "g2", 11)])
def test_msm_random_matches_oracle(gm, oracle_mod, curve, which, logn):
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = (1 << logn) + 1  # 2^k + 1: ragged chunking
    rng = rng_for(6, g.gid, logn)
    pts = o.gen_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)), nthreads=8)
    sc = random_scalars(rng, g.curve, n)
    pts[[3, n // 3, n // 2, n - 2]] = 0  # 4 infinities (multiexp_test.go:48-52)
    sc[::5, 1:] = 0                      # "smallvalues"-like: every 5th stored scalar is a single limb (multiexp_test.go:319)
    assert (_msm_gpu_affine(g, pts, sc) == o.msm_affine(pts, sc, nthreads=8)).all()


@pytest.mark.parametrize("curve,which,n", [("bn254", "g1", 64 * 157 + 37), ("bn254", "g1", 64), ("bn254", "g1", 63),
                                           ("bls12_381", "g1", 4097), ("bls12_381", "g2", 1025), ("bw6_761", "g1", 777)])
def test_msm_window_17_ragged_sizes(gm, oracle_mod, forced_options, curve, which, n):
    """Window width 17 - what every call from 2^21 points runs, with 17-bit digit codes in uint32 arrays - at sizes that are
    not a multiple of the 64-lane wave, one full wave and one short of it: random scalars (bit 16 of the code set in half of
    the digits), every fifth scalar a single limb, infinities among the points; against the oracle, and against the same
    call at c = 16 (uint16 codes)."""
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    rng = rng_for(17, g.gid, n)
    pts = o.gen_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)), nthreads=8)
    sc = random_scalars(rng, g.curve, n)
    pts[[1, n // 2, n - 1]] = 0
    sc[::5, 1:] = 0
    sc[7 % n] = 0
    want = o.msm_affine(pts, sc, nthreads=8)
    forced_options(window_bits=17)
    got17 = _msm_gpu_affine(g, pts, sc)
    forced_options(window_bits=16)
    got16 = _msm_gpu_affine(g, pts, sc)
    assert (got17 == want).all() and (got16 == want).all()


def test_msm_bn254_g1_2p20_config(gm, oracle_mod):
    """BASELINE config C2: BN254 G1, n = 2^20, against the oracle on the same seeded input."""
    g = gm.G1Affine("bn254")
    o = oracle_mod.Oracle("bn254", "g1")
    n = 1 << 20
    rng = rng_for(2, 20)
    pts = o.gen_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)), nthreads=16)
    sc = random_scalars(rng, g.curve, n)
    got = _msm_gpu_affine(g, pts, sc)
    exp = o.msm_affine(pts, sc, c=16, nthreads=16)
    assert (got == exp).all()


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g1"), ("bn254", "g2")])
def test_msm_skewed_bucket_distributions(gm, oracle_mod, curve, which):
    """Distributions that put very many points in one bucket (long partial-sum chains in the segmented accumulation):
    all scalars equal, runs of 100 equal scalars ("redundancy", multiexp_test.go:327-334), every 5th scalar = raw limb 1
    ("smallvalues", :319-325), a single repeated base, and window sizes whose top window has only a few bits."""
    import torch
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 20000 if which == "g1" else 6000
    rng = rng_for(7, g.gid)
    pts = o.gen_points(n, 12345, 999, nthreads=8)
    sc = random_scalars(rng, g.curve, n)
    equal = np.tile(sc[:1], (n, 1))
    assert (_msm_gpu_affine(g, pts, equal) == o.msm_affine(pts, equal, nthreads=8)).all()
    redundancy = np.repeat(sc[: (n + 99) // 100], 100, axis=0)[:n]
    assert (_msm_gpu_affine(g, pts, redundancy) == o.msm_affine(pts, redundancy, nthreads=8)).all()
    small = sc.copy()
    small[::5] = 0
    small[::5, 0] = 1
    assert (_msm_gpu_affine(g, pts, small) == o.msm_affine(pts, small, nthreads=8)).all()
    same_base = np.tile(pts[:1], (n, 1))
    assert (_msm_gpu_affine(g, same_base, equal) == o.msm_affine(same_base, equal, nthreads=8)).all()
    assert (_msm_gpu_affine(g, same_base, sc) == o.msm_affine(same_base, sc, nthreads=8)).all()
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    for c in (9, 12, 13, 14, 17, 20):  # the oracle, like the reference, stops at 16: the affine result does not depend on c
        w = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)
        assert (g.jac_to_affine(g.fold_windows(w, c)) == o.msm_affine(pts, sc, c=min(c, 16), nthreads=8)).all(), c


# ------------------------------------------------------------------ the reference's benchmark distributions, at benchmark size
def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", ["smallvalues", "redundancy", "value_one", "all_equal"])
def test_msm_benchmark_distribution_2p20(gm, oracle_mod, kind):
    """BenchmarkMultiExpG1's scalar distributions (multiexp_test.go:319-334) plus value-one / all-equal at 2^20 points, BN254
    G1: the crowded buckets take the multi-workgroup sort of oversized partitions (k_heavy_*) and the piece-wise long-chain
    fix-up. Closed form: bases [a_i]G built on the device, expected [sum a_i b_i]G from the oracle. The same vector through
    the host entry (point ranges + bucket merges) and over registered bases with window tables (one shared bucket set)."""
    import torch
    bench = _bench()
    g = gm.G1Jac("bn254")
    n = 1 << 20
    rng = rng_for(31, len(kind))
    a = random_scalars(rng, g.curve, n)
    b = bench.skewed_scalars(kind, random_scalars(rng, g.curve, n), g, rng)
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_b = torch.from_numpy(b.view(np.int64)).cuda()
    d_pts = torch.empty((n, g.aff_limbs), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    g.batch_scalar_mul_device(g.generator, d_a.data_ptr(), n, d_pts.data_ptr(), stream)
    expected = oracle_mod.Oracle("bn254", "g1").fixed_base_msm_affine(a, b)
    assert (g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_b.data_ptr(), n, stream)) == expected).all()
    pts = d_pts.cpu().numpy().view(np.uint64)
    jac, err = g.MultiExp(pts, b, gm.MultiExpConfig())
    assert err is None and (g.jac_to_affine(jac) == expected).all()
    rb = g.register_bases(d_points=d_pts.data_ptr(), n=n)
    try:
        rb.precompute(0)
        with gm.options(tables=2):
            assert (g.jac_to_affine(rb.multiexp_device(d_b.data_ptr(), n, stream)) == expected).all()
    finally:
        rb.release()


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_msm_crowded_buckets_all_groups(gm, oracle_mod, curve, which):
    """Crowded buckets for every group at sizes where a partition exceeds the fine sort's staging slots (so the k_heavy_*
    kernels and the piece-wise k_fixup_long run with every element type), against the oracle's MSM; several window widths
    through window_sums_device (narrow and wide fine-bucket tables), and point-range splits of the same call."""
    import torch
    bench = _bench()
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 70000 if which == "g1" and curve != "bw6_761" else 40000
    rng = rng_for(32, g.gid)
    pts = o.gen_points(n, 4242, 777, nthreads=8)
    base = random_scalars(rng, g.curve, n)
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    for kind in ("smallvalues", "value_one", "all_equal", "redundancy"):
        sc = bench.skewed_scalars(kind, base, g, rng)
        expected = o.msm_affine(pts, sc, nthreads=8)
        assert (_msm_gpu_affine(g, pts, sc) == expected).all(), kind
        d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
        for c in (8, 13, 16):
            w = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)
            assert (g.jac_to_affine(g.fold_windows(w, c)) == expected).all(), (kind, c)
    # infinities and duplicated bases inside the crowded bucket
    pts2 = pts.copy()
    pts2[::7] = 0
    pts2[1::2] = pts2[1]
    sc = bench.skewed_scalars("all_equal", base, g, rng)
    assert (_msm_gpu_affine(g, pts2, sc) == o.msm_affine(pts2, sc, nthreads=8)).all()


# ------------------------------------------------------------------ BASELINE.json configurations at their full sizes
FULL_CONFIGS = [
    ("bn254", "g1", 24),      # C3: BN254 G1 2^24
    ("bls12_381", "g1", 22),  # C4: BLS12-381 G1 2^22
    ("bls12_381", "g2", 22),  # C4: BLS12-381 G2 2^22
    ("bw6_761", "g1", 20),    # C5: BW6-761 G1 2^20
]


@pytest.mark.parametrize("curve,which,logn", FULL_CONFIGS)
def test_baseline_config_full_size(gm, oracle_mod, curve, which, logn):
    """Full-size parity for the BASELINE.json configurations: (1) bit-exact against the oracle on the same seeded input
    (the oracle runs the reference's algorithm on the host cores), (2) a size-independent property on the GPU alone:
    linearity MSM(P, s) + MSM(P, t) == MSM(P, s + t) checked through the group law of the oracle on three points."""
    import torch
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 1 << logn
    rng = rng_for(8, g.gid, logn)
    threads = 2 * gm._lib.effective_cpus()
    pts = g.generate_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)))
    # the generator is product code: spot-check it against the oracle's generator on a slice
    k0k1 = rng_for(8, g.gid, logn)
    a, b = int(k0k1.integers(1, 2**62)), int(k0k1.integers(1, 2**62))
    assert (pts[:257] == o.gen_points(257, a, b)).all()
    s = random_scalars(rng, g.curve, n)
    t = random_scalars(rng, g.curve, n)
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def gpu(sc):
        d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
        return g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream))

    ms = gpu(s)
    assert (ms == o.msm_affine(pts, s, nthreads=threads)).all()
    # linearity: s + t mod r computed limb-wise through Python ints on the stored (Montgomery) values is the Montgomery
    # form of the sum, because x -> x*R is additive
    r = g.curve.r
    nl = g.fr_limbs
    sv = sum(s[:, i].astype(object) << (64 * i) for i in range(nl))
    tv = sum(t[:, i].astype(object) << (64 * i) for i in range(nl))
    uv = (sv + tv) % r
    u = np.stack([np.array([(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in uv], dtype=np.uint64) for i in range(nl)], axis=1)
    mt, mu = gpu(t), gpu(u)
    lhs = o.jac_to_affine(o.xyzz_to_jac(o.xyzz_add_mixed(o.xyzz_add_mixed(o.xyzz_infinity(), ms), mt)))
    assert (lhs == mu).all()


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g2")])
def test_resident_bases_prefix_multiexp(gm, oracle_mod, curve, which):
    """Device-resident SRS (gmsm_bases_register): MultiExp over prefixes of the registered bases, as kzg.Commit does with
    pk.G1[:len(p)] (ecc/bn254/kzg/kzg.go:159-176), equals the oracle; more scalars than bases is the length error."""
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 3000
    rng = rng_for(9, g.gid)
    pts = o.gen_points(n, 4242, 77, nthreads=4)
    pts[11] = 0
    sc = random_scalars(rng, g.curve, n)
    rb = g.register_bases(points=pts)
    try:
        for m in (n, 1777, 1, 0):
            jac, err = rb.MultiExp(sc[:m])
            assert err is None
            assert (g.jac_to_affine(jac) == o.msm_affine(pts[:m], sc[:m])).all(), m
        _, err = rb.MultiExp(np.zeros((n + 1, g.fr_limbs), dtype=np.uint64))
        assert err == "len(points) != len(scalars)"
        _, err = rb.MultiExp(sc, gm.MultiExpConfig(NbTasks=2000))
        assert err == "invalid config: config.NbTasks > 1024"
    finally:
        rb.release()


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g2")])
def test_batch_of_multiexp_over_resident_bases(gm, oracle_mod, curve, which):
    """gmsm_multiexp_bases_batch: k scalar vectors over one registered base set (kzg.Commit of k polynomials with one SRS,
    ecc/bn254/kzg/kzg.go:159-176) from host and from device memory; every result equals the oracle's MultiExp."""
    import torch
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    nb, n, k = 5000, 4097, 5
    rng = rng_for(33, g.gid)
    pts = o.gen_points(nb, 7001, 13, nthreads=4)
    sc = np.stack([random_scalars(rng, g.curve, n) for _ in range(k)])
    sc[2] = 0                      # one all-zero vector -> infinity
    sc[3, :100] = sc[3, 100:200]   # repeated scalars
    expected = [o.msm_affine(pts[:n], sc[i]) for i in range(k)]
    rb = g.register_bases(points=pts)
    try:
        jacs, err = rb.MultiExpBatch(scalars=sc)
        assert err is None
        for i in range(k):
            assert (g.jac_to_affine(jacs[i]) == expected[i]).all(), i
        d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
        jacs, err = rb.MultiExpBatch(d_scalars=d_sc.data_ptr(), n=n, k=k, stream=torch.cuda.current_stream().cuda_stream)
        assert err is None
        for i in range(k):
            assert (g.jac_to_affine(jacs[i]) == expected[i]).all(), i
        jacs, err = rb.MultiExpBatch(scalars=sc[:1])     # k = 1
        assert err is None and (g.jac_to_affine(jacs[0]) == expected[0]).all()
        jacs, err = rb.MultiExpBatch(scalars=np.zeros((2, 0, g.fr_limbs), dtype=np.uint64))  # n = 0
        assert err is None and (g.jac_to_affine(jacs[1]) == 0).all()
        _, err = rb.MultiExpBatch(scalars=np.zeros((1, nb + 1, g.fr_limbs), dtype=np.uint64))
        assert err == "len(points) != len(scalars)"
    finally:
        rb.release()


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bn254", "g2"), ("bls12_381", "g1"), ("bw6_761", "g2")])
def test_fold_matches_reference_definition(gm, oracle_mod, curve, which):
    """Fold (ecc/bn254/multiexp.go:320-340): sum_i points[i] * coeff^i. Expected value: the oracle's MultiExp over the
    powers 1, g, g^2, ... built with the oracle's own fr multiplication (and cross-checked with Python integers)."""
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    cv = g.curve
    Fr = oracle_mod.Field(f"{cv.name}_fr", cv.fr_limbs)
    rng = rng_for(27, g.gid)
    for n in (0, 1, 2, 150):
        pts = o.gen_points(max(n, 1), 31, 7, nthreads=2)[:n]
        coeff = random_scalars(rng, cv, 1)[0]
        powers = np.zeros((n, cv.fr_limbs), dtype=np.uint64)
        acc = scalars_from_ints(cv, [1])[0]
        for i in range(n):
            powers[i] = acc
            acc = Fr.mul(acc, coeff)
        if n:
            gamma = sum(int(v) << (64 * k) for k, v in enumerate(Fr.from_mont(coeff)))
            last = sum(int(v) << (64 * k) for k, v in enumerate(Fr.from_mont(powers[-1])))
            assert last == pow(gamma, n - 1, cv.r)
        expected = o.msm_affine(pts, powers) if n else np.zeros(g.aff_limbs, dtype=np.uint64)
        aff, err = g.Fold(pts, coeff)
        assert err is None
        assert (aff == expected).all(), n
    _, err = g.Fold(pts, coeff, gm.MultiExpConfig(NbTasks=1025))
    assert err == "invalid config: config.NbTasks > 1024"


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g2"), ("bw6_761", "g1")])
@pytest.mark.parametrize("mode", ["windows", "points"])
def test_sharded_exchange_pieces_on_one_gpu(gm, oracle_mod, curve, which, mode):
    """What bench.py runs on N GPUs, rank by rank on one GPU: gmsm_window_sums_enqueue leaves each rank's totals in a device
    buffer (no copy-back), the buffers are concatenated exactly as all_gather_into_tensor does, and the host folds them
    (window decomposition: gmsm_fold_windows; point decomposition: gmsm_fold_window_sets). World sizes 1, 2, 3, 8 with an
    n that does not divide evenly, host bases and registered slices, must all equal the oracle."""
    import importlib
    import torch
    sharding = importlib.import_module("gnark-crypto_amd.sharding")
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 4099
    rng = rng_for(23, g.gid)
    pts = o.gen_points(n, 2024, 9, nthreads=4)
    pts[5] = 0
    sc = random_scalars(rng, g.curve, n)
    sc[17] = 0
    expected = o.msm_affine(pts, sc, nthreads=4)
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for world in (1, 2, 3, 8):
        for use_resident in (False, True):
            plans = [sharding.shard_plan(g, n, r, world, mode) for r in range(world)]
            rows = plans[0]["rows"]
            gathered = torch.zeros((world * rows, g.xyzz_limbs), dtype=torch.int64, device="cuda")
            handles = []
            for r, p in enumerate(plans):
                lo, hi = p["lo"], p["hi"]
                rb = g.register_bases(d_points=d_pts[lo:hi].data_ptr(), n=hi - lo) if use_resident else None
                handles.append(rb)
                g.window_sums_enqueue(d_pts[lo:hi].data_ptr(), d_sc[lo:hi].data_ptr(), hi - lo, p["c"], p["win_first"],
                                      p["win_stride"], stream, gathered[r * rows:(r + 1) * rows].data_ptr(), bases=rb)
            host = gathered.cpu().numpy().view(np.uint64).reshape(world, rows, g.xyzz_limbs)
            for rb in handles:
                if rb is not None:
                    rb.release()
            if mode == "points":
                jac = g.fold_window_sets(host, plans[0]["c"])
            else:
                jac = g.fold_windows(sharding.unpack_gathered(host, plans[0]["nwin"], world, g.xyzz_limbs), plans[0]["c"])
            assert (g.jac_to_affine(jac) == expected).all(), (world, use_resident)


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g2")])
def test_two_multiexp_in_flight(gm, oracle_mod, curve, which):
    """gmsm_multiexp_bases_submit / gmsm_multiexp_collect: two MultiExp calls over the same resident bases in flight on
    two workspaces (the GPU-side counterpart of BenchmarkManyMultiExpG1Reference, ecc/bn254/multiexp_test.go:385-415).
    Every result equals the oracle whatever the collection order; a third submit and a repeated ticket are refused;
    synchronous calls go through whether one or two tickets are outstanding (three workspaces, tickets hold at most two)."""
    import torch
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 6000
    rng = rng_for(21, g.gid)
    pts = o.gen_points(n, 555, 99, nthreads=4)
    sets = [(random_scalars(rng, g.curve, m), m) for m in (n, 4321, n, 17, 0, n)]
    expect = [o.msm_affine(pts[:m], sc) for sc, m in sets]
    d_sc = [torch.from_numpy(sc.view(np.int64).copy()).cuda() if m else torch.zeros(4, dtype=torch.int64).cuda() for sc, m in sets]
    torch.cuda.synchronize()
    rb = g.register_bases(points=pts)
    try:
        # rolling pipeline, depth 2, in-order collection
        prev = None
        got = []
        for i, (_, m) in enumerate(sets):
            t = rb.submit(d_sc[i].data_ptr(), m)
            if prev is not None:
                got.append(rb.collect(prev))
            prev = t
        got.append(rb.collect(prev))
        for i, jac in enumerate(got):
            assert (g.jac_to_affine(jac) == expect[i]).all(), i
        # out-of-order collection + refusals
        t0 = rb.submit(d_sc[0].data_ptr(), sets[0][1])
        jac_sync = rb.multiexp_device(d_sc[1].data_ptr(), sets[1][1])  # one slot busy: the other one serves
        assert (g.jac_to_affine(jac_sync) == expect[1]).all()
        t1 = rb.submit(d_sc[1].data_ptr(), sets[1][1], stream=torch.cuda.current_stream().cuda_stream)
        with pytest.raises(RuntimeError, match="two submitted MultiExp calls are outstanding"):
            rb.submit(d_sc[2].data_ptr(), sets[2][1])
        # two tickets outstanding: a blocking call still goes through at once (the third workspace, which tickets can
        # never hold) - round 3 gave up here after two seconds, whoever held the tickets
        jac_sync = rb.multiexp_device(d_sc[2].data_ptr(), sets[2][1])
        assert (g.jac_to_affine(jac_sync) == expect[2]).all()
        jac, err = rb.MultiExp(sets[3][0])
        assert err is None and (g.jac_to_affine(jac) == expect[3]).all()
        assert (g.jac_to_affine(rb.collect(t1)) == expect[1]).all()
        with pytest.raises(RuntimeError, match="ticket"):
            rb.collect(t1)
        assert (g.jac_to_affine(rb.collect(t0)) == expect[0]).all()
        with pytest.raises(RuntimeError, match="ticket"):
            rb.collect(12345)
        # everything is free again
        jac, err = rb.MultiExp(sets[3][0])
        assert err is None and (g.jac_to_affine(jac) == expect[3]).all()
    finally:
        rb.release()


@pytest.mark.parametrize("curve,which,c", [("bn254", "g1", 16), ("bn254", "g1", 13), ("bls12_381", "g2", 16)])
def test_window_sharded_pieces_on_one_gpu(gm, oracle_mod, curve, which, c):
    """The multi-GPU decomposition executed rank by rank on one GPU: every "rank" computes the totals of its own windows
    (gmsm_window_sums_device with win_first = rank, win_stride = world), the pieces are merged like the RCCL all-gather
    does (gnark-crypto_amd/sharding.py) and folded; world sizes 2, 3, 8 (uneven ownership) must all equal the oracle."""
    import importlib
    import torch
    sharding = importlib.import_module("gnark-crypto_amd.sharding")
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    n = 5000
    rng = rng_for(10, g.gid, c)
    pts = o.gen_points(n, 31337, 101, nthreads=4)
    sc = random_scalars(rng, g.curve, n)
    expected = o.msm_affine(pts, sc, c=c, nthreads=4)
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    nwin = g.num_windows(c)
    for world in (2, 3, 8):
        gathered = np.stack([
            sharding.pack_local(g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c, rank, world), nwin, world, g.xyzz_limbs)
            for rank in range(world)])
        totals = sharding.unpack_gathered(gathered, nwin, world, g.xyzz_limbs)
        assert (g.jac_to_affine(g.fold_windows(totals, c)) == expected).all(), world


def test_concurrent_multiexp_calls(gm, oracle_mod):
    """The C ABI is re-entrant: three MultiExp calls in flight from different OS threads (BenchmarkManyMultiExpG1Reference,
    multiexp_test.go:385-415) each return their own correct result."""
    import threading
    g = gm.G1Affine("bn254")
    o = oracle_mod.Oracle("bn254", "g1")
    n = 20000
    jobs = []
    for j in range(3):
        rng = rng_for(11, j)
        pts = o.gen_points(n, 1000 + j, 17 + j, nthreads=4)
        sc = random_scalars(rng, g.curve, n)
        jobs.append((pts, sc, o.msm_affine(pts, sc, nthreads=4)))
    results = [None] * 3

    def run(j):
        for _ in range(5):
            results[j] = g.MultiExp(jobs[j][0], jobs[j][1])

    threads = [threading.Thread(target=run, args=(j,)) for j in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for j in range(3):
        aff, err = results[j]
        assert err is None and (aff == jobs[j][2]).all(), j


def test_mixed_entries_from_many_threads(gm, oracle_mod):
    """Five OS threads hammer one device at once through DIFFERENT entries and groups - host-pointer MultiExp (BN254 G1),
    registered bases with host scalars (BLS12-381 G1), the device entry (BN254 G2), a submit/collect pipeline and the
    fixed-base batch - while another thread toggles the stage profiler. Two workspaces are shared by all of them (leases);
    every single result must be the oracle's."""
    import threading
    import torch
    errors = []
    lib = gm._lib.load()

    def check(name, got, want):
        if not (np.asarray(got) == np.asarray(want)).all():
            errors.append(name)

    def host_g1():
        g, o = gm.G1Affine("bn254"), oracle_mod.Oracle("bn254", "g1")
        for it in range(6):
            n = 1500 + 700 * it
            pts = o.gen_points(n, 11 + it, 3)
            sc = random_scalars(rng_for(61, it), g.curve, n)
            aff, err = g.MultiExp(pts, sc)
            if err is not None:
                errors.append("host_g1 " + err)
            else:
                check(f"host_g1 {it}", aff, o.msm_affine(pts, sc))

    def resident_bls():
        g, o = gm.G1Affine("bls12_381"), oracle_mod.Oracle("bls12_381", "g1")
        pts = o.gen_points(4000, 5, 9)
        rb = g.register_bases(points=pts)
        try:
            for it in range(6):
                m = 4000 - 555 * it
                sc = random_scalars(rng_for(62, it), g.curve, m)
                jac, err = rb.MultiExp(sc)
                if err is not None:
                    errors.append("resident_bls " + err)
                else:
                    check(f"resident_bls {it}", g.jac_to_affine(jac), o.msm_affine(pts[:m], sc))
        finally:
            rb.release()

    def device_g2():
        g, o = gm.G2Affine("bn254"), oracle_mod.Oracle("bn254", "g2")
        n = 1200
        pts = o.gen_points(n, 21, 4)
        d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
        for it in range(5):
            sc = random_scalars(rng_for(63, it), g.curve, n)
            d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
            torch.cuda.synchronize()
            jac = g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n)
            check(f"device_g2 {it}", g.jac_to_affine(jac), o.msm_affine(pts, sc))

    def pipeline_g1():
        g, o = gm.G1Affine("bn254"), oracle_mod.Oracle("bn254", "g1")
        n = 5000
        pts = o.gen_points(n, 31, 7)
        rb = g.register_bases(points=pts)
        try:
            scs = [random_scalars(rng_for(64, it), g.curve, n) for it in range(6)]
            d = [torch.from_numpy(sc.view(np.int64)).cuda() for sc in scs]
            torch.cuda.synchronize()
            prev, got = None, []
            for it in range(6):
                while True:  # both workspaces may be leased by the other threads for a moment
                    try:
                        t = rb.submit(d[it].data_ptr(), n)
                        break
                    except RuntimeError:
                        if prev is not None:
                            got.append(rb.collect(prev))
                            prev = None
                if prev is not None:
                    got.append(rb.collect(prev))
                prev = t
            got.append(rb.collect(prev))
            for it, jac in enumerate(got):
                check(f"pipeline_g1 {it}", g.jac_to_affine(jac), o.msm_affine(pts, scs[it]))
        finally:
            rb.release()

    def fixed_base():
        g, o = gm.G1Affine("bn254"), oracle_mod.Oracle("bn254", "g1")
        for it in range(4):
            n = 800 + 100 * it
            sc = scalars_from_ints(g.curve, [(5 + it + i * 977) % g.curve.r for i in range(n)])
            check(f"fixed_base {it}", g.BatchScalarMultiplication(o.generator, sc), o.gen_points(n, 5 + it, 977))

    stop = threading.Event()

    def profiler():
        while not stop.is_set():
            lib.gmsm_set_profiling(1)
            stop.wait(0.01)
            lib.gmsm_set_profiling(0)
            stop.wait(0.01)

    workers = [threading.Thread(target=f) for f in (host_g1, resident_bls, device_g2, pipeline_g1, fixed_base)]
    prof = threading.Thread(target=profiler)
    prof.start()
    for t in workers:
        t.start()
    for t in workers:
        t.join(timeout=600)
    stop.set()
    prof.join()
    lib.gmsm_set_profiling(0)
    assert not any(t.is_alive() for t in workers), "a worker thread is stuck"
    assert errors == [], errors


# ------------------------------------------------------------------ N3: fixed-base batch
@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bn254", "g2"), ("bls12_381", "g1"), ("bls12_381", "g2"),
                                         ("bw6_761", "g1")])
def test_batch_scalar_multiplication(gm, oracle_mod, curve, which):
    """BatchScalarMultiplicationG1/G2 (ecc/bn254/g1.go:1039-1118) on the device: scalars k0 + i*k1 against the oracle's
    incremental point generator, random and edge scalars (0, 1, 2, r-1, 2^c-1 patterns) against the oracle's
    double-and-add, a non-generator base, and the point at infinity as base."""
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    cv = g.curve
    n = 3000 if which == "g1" else 700
    k0, k1 = 0x1234567 + (cv.r >> 3), 0x9e3779b97f4a7c15
    ks = [(k0 + i * k1) % cv.r for i in range(n)]
    sc = scalars_from_ints(cv, ks)
    expected = o.gen_points(n, k0, k1, nthreads=4)
    got = g.BatchScalarMultiplication(o.generator, sc)
    assert (got == expected).all()
    # edge and random scalars on another base
    base = expected[7]
    rng = rng_for(41, g.gid)
    edge = [0, 1, 2, cv.r - 1, cv.r - 2, 255, 256, 127, 128, 129, (1 << 64) - 1, 1 << 64, (1 << 200) + 1]
    rnd = [int.from_bytes(rng.bytes(48), "little") % cv.r for _ in range(40)]
    vals = edge + rnd
    got = g.BatchScalarMultiplication(base, scalars_from_ints(cv, vals))
    for i, k in enumerate(vals):
        exp = o.jac_to_affine(o.scalar_mul(base, k)) if k else np.zeros(g.aff_limbs, dtype=np.uint64)
        assert (got[i] == exp).all(), (i, hex(k))
    # infinity base, empty batch
    assert (g.BatchScalarMultiplication(np.zeros(g.aff_limbs, dtype=np.uint64), sc[:10]) == 0).all()
    assert g.BatchScalarMultiplication(base, sc[:0]).shape == (0, g.aff_limbs)


def test_batch_scalar_multiplication_large_table(gm, oracle_mod, forced_options):
    """The larger table (c = 11, chosen from 2^21 scalars on) on a size the oracle checks in seconds."""
    forced_options(fixed_base_bits=11)
    g = _group(gm, "bn254", "g1")
    o = oracle_mod.Oracle("bn254", "g1")
    n = 20000
    k0, k1 = 77, (1 << 250) + 12345
    sc = scalars_from_ints(g.curve, [(k0 + i * k1) % g.curve.r for i in range(n)])
    assert (g.BatchScalarMultiplication(o.generator, sc) == o.gen_points(n, k0, k1, nthreads=4)).all()


@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g2"), ("bw6_761", "g1")])
def test_batch_jacobian_to_affine(gm, oracle_mod, curve, which):
    """BatchJacobianToAffineG1 (ecc/bn254/g1.go:989-1035): Jacobian points with non-trivial Z (outputs of the oracle's
    double-and-add), with infinities (Z = 0) sprinkled in, against the oracle's FromJacobian one by one."""
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    rng = rng_for(43, g.gid)
    n = 150
    jac = np.zeros((n, g.jac_limbs), dtype=np.uint64)
    for i in range(n):
        if i % 17 == 5:
            continue  # infinity: Z = 0 (X, Y arbitrary)
        jac[i] = o.scalar_mul(o.generator, int.from_bytes(rng.bytes(40), "little") % g.curve.r)
    jac[5, : g.jac_limbs // 3] = 7  # garbage X with Z = 0 must still give (0, 0)
    got = g.BatchJacobianToAffine(jac)
    for i in range(n):
        assert (got[i] == o.jac_to_affine(jac[i])).all(), i
    assert g.BatchJacobianToAffine(jac[:0]).shape == (0, g.aff_limbs)


# ------------------------------------------------------------------ the boundary from plain C (what cgo would bind)
@pytest.mark.parametrize("curve,which", [("bn254", "g1"), ("bls12_381", "g2"), ("bw6_761", "g1")])
def test_c_client_through_the_abi(gm, oracle_mod, curve, which, tmp_path):
    """tests/c/abi_client.c is compiled with gcc against include/gmsm.h and linked to libgmsm.so only - no Python, no torch
    in the process: the per-curve drop-in symbol, gmsm_multiexp_affine, the registered-bases entry and bases registered from their
    compressed encoding must all return the oracle's affine point; the two argument errors must come back as the documented codes."""
    import os
    import subprocess
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "gnark-crypto_amd", "csrc")
    exe = str(tmp_path / "abi_client")
    subprocess.run(["gcc", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "abi_client.c"), "-o", exe,
                    "-L", libdir, "-lgmsm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    n = 2500
    rng = rng_for(51, g.gid)
    pts = o.gen_points(n, 4711, 3, nthreads=4)
    pts[100] = 0
    sc = random_scalars(rng, g.curve, n)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([n, g.aff_limbs, g.fr_limbs], dtype=np.uint64).tofile(f)
        pts.tofile(f)
        sc.tofile(f)
    env = dict(os.environ)
    env.pop("GMSM_LIB", None)
    r = subprocess.run([exe, str(g.gid), fin, fout], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = np.fromfile(fout, dtype=np.uint64)
    expected = o.msm_affine(pts, sc, nthreads=4)
    for i in range(4):  # drop-in symbol, affine entry, registered bases, bases through the compressed wire format
        assert (out[i * g.aff_limbs:(i + 1) * g.aff_limbs] == expected).all(), i
    assert out[4 * g.aff_limbs] == gm._lib.GMSM_ERR_LEN and out[4 * g.aff_limbs + 1] == gm._lib.GMSM_ERR_CONFIG


@pytest.mark.parametrize("curve,which,budget", [("bn254", "g1", 12.0), ("bls12_381", "g1", 8.0), ("bn254", "g2", 8.0)])
def test_bounded_fuzz_against_the_oracle(gm, oracle_mod, curve, which, budget):
    """tools/fuzz_parity.py inside the suite, bounded in time (~30 s for the three groups): random sizes, eight input
    distributions (uniform, small, few distinct, all equal, sparse, powers of two and r - k, one base repeated - P + P in
    buckets and in the reduction -, every base twice with s and r - s - P - P everywhere, result infinity) and five entry
    points (drop-in, registered bases, submit/collect, batch, the in-library sharded entry with 2-5 logical ranks in either
    decomposition) against the oracle. (Round 3, 40 s per group on all six groups: 3581 cases, 0 mismatches.)"""
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([_sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), str(budget), curve, which],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 mismatches" in r.stdout


def test_bn254_g1_2_pow_26_closed_form(gm, oracle_mod):
    """The largest size north_star names (2^26 points, 4 GiB of bases), checked through the closed form: bases [a_i]G
    built on the device, result must be [sum a_i b_i]G (shape of multiexp_test.go:54-60). The a_i, b_i repeat with period
    2^22 to keep the host side of the test short; the MSM itself sees 2^26 distinct (point, scalar) pairs only through
    their positions, so the 16 blocks additionally check that equal inputs at different indices add up: result = 16 x
    the 2^22 closed form."""
    import torch
    g = gm.G1Jac("bn254")
    o = oracle_mod.Oracle("bn254", "g1")
    m, reps = 1 << 22, 16
    rng = rng_for(26, 1)
    a = random_scalars(rng, g.curve, m)
    b = random_scalars(rng, g.curve, m)
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_blk = torch.empty((m, g.aff_limbs), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    g.batch_scalar_mul_device(g.generator, d_a.data_ptr(), m, d_blk.data_ptr(), stream)
    d_pts = d_blk.repeat(reps, 1).contiguous()
    d_sc = torch.from_numpy(b.view(np.int64)).cuda().repeat(reps, 1).contiguous()
    n = m * reps
    assert n == 1 << 26
    jac = g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream)
    fr = oracle_mod.Field("bn254_fr", 4)
    k_limbs = fr.from_mont(fr.dot(a, b))
    k = sum(int(v) << (64 * i) for i, v in enumerate(k_limbs)) * reps % g.curve.r
    expected = o.jac_to_affine(o.scalar_mul(o.generator, k))
    assert (g.jac_to_affine(jac) == expected).all()
    del d_pts, d_sc, d_blk, d_a
    torch.cuda.empty_cache()
