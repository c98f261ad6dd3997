"""The bucket reduction (k_reduce_serial / k_reduce_serial_q, k_combine_q / k_combine_we, k_reduce2_q) at launch shapes forced
through GMSM_OPT_REDUCE_SHAPE, over bucket contents chosen by tests/reduce_cases.py - tests/test_reduce_cases_model.py shows
on the host model that every case meets P + P, P - P or the infinite operand it is named for at every shape used here.

Bucket j of window w is filled through the real pipeline: an entry with the scalar (j + 1) 2^(c w) and the base [k]G puts [k]G
into it with no carry; two entries per bucket (k1 + k2 = b) leave a record with zz != 1, k2 = -k1 one that is stored but
infinite. The last bucket is reached through the digit -2^(c-1), which carries into window w + 1. Three windows are filled: the
first, a middle one and the last but one. Every window total of window_sums_device (all windows at once, and the middle one
alone: nw = 1) must be [sum_i digit_w(s_i) k_i]G, limb for limb after the oracle's conversion to affine: the digits are the
reference's decomposition (oracle.partition_scalars), the point is the big-integer model's (pyref). Windows without entries
and sums that vanish must come back as infinity (zz = 0).

Shapes: c in 2, 7, 11, 14 - 2^(c-1) = 2, 64, 1024, 8192 reachable buckets (the bucket set itself is 2^(max(c, lastC) - 1)
buckets, as the reference sizes it: 4 for BN254 at c = 2, whose top window is a full one) - the smallest with L above the
bucket count, one ragged combine block, several blocks, enough blocks for three levels at small L; log2L in 1, 2, 4, 8; two and
three levels wherever the planner can form them without raising log2L (two: NB <= 64 * 64 L, three: NB > 64 L); k_combine_q,
and k_combine_we for the group that has it. Every forced shape is checked against gmsm_debug_reduce_shape. BW6-761 keeps
c = 14 (its case takes 6 to 7 s on an MI355X, the others 0.5 to 3 s).

The two other forms of the buckets, at one two-level and one three-level shape per group: merged point ranges (GMSM_OPT_MAX_RUN:
every record stored, no start offsets) and the shared bucket set of window tables - by value, [sum s_i k_i]G."""
import numpy as np
import pytest

import reduce_cases as rc
from conftest import ALL_GROUPS

pytestmark = pytest.mark.gpu

NW = 3               # populated windows
ONE_ENTRY = ("sparse", "single")   # cases whose buckets hold one entry; the others two (a record with zz != 1)
_CACHE = {}          # (group, c, contents) -> inputs and expected totals, kept for the shapes of one test: neither depends on the shape


def small_runs(gm):
    return int(gm._lib.load().gmsm_debug_small_runs())


def groups(gm, oracle_mod, pyref_mod, curve, which):
    g = (gm.G1Jac if which == "g1" else gm.G2Jac)(curve)
    return g, oracle_mod.Oracle(curve, which), pyref_mod.Group(g.curve, which)


def nbuckets(g, c):
    return rc.nbuckets(g.curve.fr_bits, c)


def limbs_from_ints(curve, values):
    """conftest.scalars_from_ints for tens of thousands of values: Montgomery form, little-endian uint64 limbs"""
    R, r, nb = curve.fr_R, curve.r, 8 * curve.fr_limbs
    raw = b"".join((v % r * R % r).to_bytes(nb, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, curve.fr_limbs).copy()


def filled_windows(g, c):
    nwin = g.num_windows(c)
    ws = [0, nwin // 2, nwin - 2]  # the last but one is the last full-width window whose carry has a window to go to
    assert len(set(ws)) == NW and all(w + 1 not in ws for w in ws) and (nwin - 1) * c < g.curve.fr_bits
    return ws


def entries(g, c, case):
    """(scalars, base multipliers) as integers: bucket j of the k-th filled window holds case.b[k][j]"""
    import random
    r = g.curve.r
    rng = random.Random(f"entries/{g.gid}/{c}/{case.name}")
    two = case.name.split("@")[0] not in ONE_ENTRY
    ss, ks = [], []
    for w, b, inf in zip(filled_windows(g, c), case.b, case.inf):
        for j, (v, stored_inf) in enumerate(zip(b, inf)):
            if not v and not stored_inf:
                continue
            top = j + 1 == 1 << (c - 1)  # digit -2^(c-1): the bucket receives the negated base
            parts = [v]
            if stored_inf or two:
                k1 = rng.randrange(1, r)
                parts = [k1, (v - k1) % r]
            for k in parts:
                if k:
                    ss.append((j + 1) << (c * w))
                    ks.append((r - k) if top else k)
    return ss, ks


def prepared(gm, g, o, pg, c, case):
    """device inputs and the expected affine total of every window (None: infinity), made once per contents"""
    import torch
    key = (g.gid, c, case.key())
    if key not in _CACHE:
        r = g.curve.r
        ss, ks = entries(g, c, case)
        assert ss and max(ss) < r
        sc = limbs_from_ints(g.curve, ss)
        pts = g.BatchScalarMultiplication(g.generator, limbs_from_ints(g.curve, ks))
        codes = o.partition_scalars(sc, c).astype(np.int64)
        digits = np.where(codes & 1, -((codes >> 1) + 1), codes >> 1)
        sums = []
        for w in range(digits.shape[0]):
            idx = np.nonzero(digits[w])[0]
            sums.append(sum(int(digits[w, i]) * ks[i] for i in idx) % r if idx.size else None)
        # the carries aside, the filled windows hold what the case says
        for w, b in zip(filled_windows(g, c), case.b):
            assert sums[w] == rc.weighted(r, b) or (sums[w] is None and not any(b))
        want = [None if not s else np.array(pg.point_to_limbs(pg.mul(s, pg.gen)), dtype=np.uint64) for s in sums]
        full = sum(s * k for s, k in zip(ss, ks)) % r
        whole = np.array(pg.point_to_limbs(pg.mul(full, pg.gen) if full else None), dtype=np.uint64)
        d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
        d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
        _CACHE[key] = (len(ss), pts, sc, d_pts, d_sc, want, whole)
    return _CACHE[key]


def check_totals(g, o, totals, want, windows, tag):
    cl = g.coord_limbs
    for row, w in zip(totals, windows):
        zz = row[2 * cl:3 * cl]
        if want[w] is None:
            assert not zz.any(), (tag, w, "expected infinity")
        else:
            assert zz.any(), (tag, w, "infinity")
            assert (o.jac_to_affine(o.xyzz_to_jac(row)) == want[w]).all(), (tag, w)


def combine_kernels(gm, g, NB):
    """the combine kernels gmsm_debug_reduce_shape reports as available when each is asked for"""
    out = []
    for k in (1, 2):
        with gm.options(reduce_shape=k << 6):
            if g.reduce_shape(1, NB)["combine"] == k:
                out.append(k)
    assert out[0] == 1 and g.reduce_shape(1, NB)["combine"] in (1, 2)
    return out


def force(forced_options, gm, g, nw, NB, log2L, levels, kernel):
    """force the shape and require that the planner reports exactly it"""
    forced_options(reduce_shape=log2L | levels << 4 | kernel << 6)
    got = g.reduce_shape(nw, NB)
    L = 1 << log2L
    blocks1 = -(-NB // (64 * L))
    assert got["log2L"] == log2L and got["nblocks1"] == blocks1 and got["combine"] == kernel, (got, nw, NB, log2L, levels, kernel)
    assert got["nblocks2"] == (-(-blocks1 // 64) if levels == 3 else 0), (got, nw, NB, log2L, levels)
    last = got["nblocks2"] or blocks1
    assert got["active"] == max(2, 1 << (last - 1).bit_length()) and got["active"] <= 64
    return got


RUN_LOG = {}  # group -> shapes run (printed by the last test of the file: pytest -s)


@pytest.mark.parametrize("c", rc.C_VALUES)
@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_reduction_at_forced_shapes(gm, oracle_mod, pyref_mod, forced_options, curve, which, c):
    g, o, pg = groups(gm, oracle_mod, pyref_mod, curve, which)
    _CACHE.clear()
    forced_options(glv=0)
    r, NB, NBc = g.curve.r, nbuckets(g, c), 1 << (c - 1)
    assert NB == NBc or (curve, c) == ("bn254", 2)
    nwin = g.num_windows(c)
    mid = filled_windows(g, c)[1]
    kernels = combine_kernels(gm, g, NB)
    assert (2 in kernels) == ((curve, which) == ("bn254", "g1"))
    shapes = rc.shapes(NB)
    assert shapes and all(rc.admissible(NB, l2, lv) for l2, lv in shapes)
    small = small_runs(gm)
    for log2L, levels in shapes:
        for name, case in rc.cases(r, NBc, log2L, levels, NW).items():
            n, _, _, d_pts, d_sc, want, _ = prepared(gm, g, o, pg, c, case)
            for kernel in kernels:
                tag = (name, log2L, levels, kernel)
                got = force(forced_options, gm, g, nwin, NB, log2L, levels, kernel)
                RUN_LOG.setdefault((curve, which), set()).add((NB, log2L, levels, kernel, got["serial_quad"]))
                totals = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)
                assert totals.shape[0] == nwin
                check_totals(g, o, totals, want, range(nwin), tag)
                force(forced_options, gm, g, 1, NB, log2L, levels, kernel)
                one = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c, win_first=mid, win_stride=nwin)
                assert one.shape[0] == 1
                check_totals(g, o, one, want, [mid], tag + ("nw=1",))
    assert small_runs(gm) == small, "the fused small-n kernel took a call"


OTHER_FORMS_C = 11  # 1024 buckets: log2L = 1 has two-level and three-level shapes


@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_merged_ranges_and_shared_bucket_set_at_forced_shapes(gm, oracle_mod, pyref_mod, forced_options, curve, which, levels):
    """the same vectors where every record is stored (point ranges merged by k_merge_buckets: starts == nullptr) and over the
    one bucket set of window tables, whose buckets hold the entries of all windows"""
    g, o, pg = groups(gm, oracle_mod, pyref_mod, curve, which)
    c, log2L = OTHER_FORMS_C, 1
    _CACHE.clear()
    r, NB = g.curve.r, nbuckets(g, c)
    assert rc.admissible(NB, log2L, levels)
    forced_options(glv=0, small_bits=1, window_bits=c)
    small = small_runs(gm)
    named = rc.cases(r, NB, log2L, levels, NW)
    for kernel in combine_kernels(gm, g, NB):
        for name in ("dense", "alternating", "zero_S", "zero_total", "finish+", "finish-", "finish2+", "finish2-", "stored_infinity"):
            n, pts, sc, d_pts, d_sc, _, whole = prepared(gm, g, o, pg, c, named[name])
            force(forced_options, gm, g, g.num_windows(c), NB, log2L, levels, kernel)
            with gm.options(max_run=max(1, n // 3)):
                got = g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n))
            assert (got == whole).all(), ("merged ranges", name, kernel)
            if name in ("dense", "stored_infinity", "zero_total"):
                force(forced_options, gm, g, 1, NB, log2L, levels, kernel)
                rb = g.register_bases(points=pts)
                try:
                    assert rb.precompute(c) == c
                    runs = int(gm._lib.load().gmsm_debug_table_runs())
                    with gm.options(tables=2):
                        got = g.jac_to_affine(rb.multiexp_device(d_sc.data_ptr(), n))
                    assert int(gm._lib.load().gmsm_debug_table_runs()) == runs + 1
                    assert (got == whole).all(), ("window tables", name, kernel)
                finally:
                    rb.release()
    assert small_runs(gm) == small, "the fused small-n kernel took a call"


def test_options_are_back_and_shapes_are_listed(gm):
    assert gm.get_option("reduce_shape") == 0
    for grp, shapes in sorted(RUN_LOG.items()):
        print(grp, "(NB, log2L, levels, combine kernel, serial on quads):", sorted(shapes))
