"""The reduction's host tail (GMSM_OPT_REDUCE_TAIL = 2: k_combine_we without its tail, k_plane_sums, GroupHost::fold_planes)
against the device ladder (= 1) and the big-integer model, BN254 G1 - the group that has the plane kernels.

Buckets are filled through the real pipeline with the generators of tests/reduce_cases.py exactly as
tests/test_gpu_reduce_shapes.py fills them (its helpers are imported): three populated windows, bucket j of a window holds
[b_j]G, two entries per bucket where the case asks for a record with zz != 1, k and -k for a stored infinite record, the last
bucket through the carry digit. Shapes (forced through GMSM_OPT_REDUCE_SHAPE, which the option at 2 does not mind, so that
the middle window alone runs the same shape as all windows): c = 11 with L = 32 (one ragged combine block of 32 pairs: 7 planes
per window), c = 13 with L = 32 (two blocks: 8 planes), c = 16 with L = 8 (64 blocks: 13 planes) and c = 16 with L = 4 and
three levels (128 blocks, as many as the headline has and the most k_plane_sums takes: 14 planes; the ladder runs a second
combine there). Families: sparse and single buckets at the seams, P + P (all_equal: every
pair sum adds equal operands; finish+), P - P and stored infinite records (alternating, stored_infinity, finish-, zero_total).

Every case, all windows at once and the middle window alone (nw = 1):
  - the window totals of both forms equal the model's, affine limb for limb, and therefore each other;
  - the folded MultiExp of both forms equals [sum s_i k_i]G;
  - gmsm_debug_plane_runs counts exactly the runs of the host form; gmsm_debug_reduce_shape does not depend on the option.
With the option at 0 a forced GMSM_OPT_REDUCE_SHAPE keeps the ladder, and a plain 2^12-point call takes the host form."""
import numpy as np
import pytest

import reduce_cases as rc
import test_gpu_reduce_shapes as shapes_test

pytestmark = pytest.mark.gpu

SHAPES = {  # label: (c, log2L, levels, first-level blocks, case families)
    "c11": (11, 5, 2, 1, ("sparse", "single", "all_equal", "alternating", "stored_infinity", "finish+", "finish-", "zero_total")),
    "c13": (13, 5, 2, 2, ("sparse", "single", "all_equal", "stored_infinity", "finish+", "finish-")),
    "c16": (16, 3, 2, 64, ("sparse", "single", "all_equal", "stored_infinity")),
    "c16x128": (16, 2, 3, 128, ("sparse", "single", "all_equal", "stored_infinity")),
}


def plane_runs(gm):
    return int(gm._lib.load().gmsm_debug_plane_runs())


@pytest.mark.parametrize("label,family", [(k, f) for k, v in SHAPES.items() for f in v[4]])
def test_host_tail_matches_ladder_and_model(gm, oracle_mod, pyref_mod, forced_options, label, family):
    c, log2L, levels, blocks, _ = SHAPES[label]
    g, o, pg = shapes_test.groups(gm, oracle_mod, pyref_mod, "bn254", "g1")
    shapes_test._CACHE.clear()
    forced_options(glv=0, small_bits=1, window_bits=c)
    r, NB, nwin = g.curve.r, shapes_test.nbuckets(g, c), g.num_windows(c)
    mid = shapes_test.filled_windows(g, c)[1]
    shape = shapes_test.force(forced_options, gm, g, nwin, NB, log2L, levels, 2)
    assert shape["nblocks1"] == blocks and shapes_test.force(forced_options, gm, g, 1, NB, log2L, levels, 2)["nblocks1"] == blocks
    named = rc.cases(r, 1 << (c - 1), log2L, levels, shapes_test.NW)
    picked = [n for n in named if n == family or n.split("@")[0] == family]
    assert picked
    for name in picked:
        n, _, _, d_pts, d_sc, want, whole = shapes_test.prepared(gm, g, o, pg, c, named[name])
        got = {}
        for tail in (1, 2):
            forced_options(reduce_tail=tail)
            assert g.reduce_shape(nwin, NB) == shape
            runs = plane_runs(gm)
            totals = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)
            assert totals.shape[0] == nwin
            shapes_test.check_totals(g, o, totals, want, range(nwin), (name, tail))
            one = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c, win_first=mid, win_stride=nwin)
            shapes_test.check_totals(g, o, one, want, [mid], (name, tail, "nw=1"))
            got[tail] = g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n))
            assert (got[tail] == whole).all(), (name, tail)
            assert plane_runs(gm) == runs + (3 if tail == 2 else 0), (name, tail)
        assert (got[1] == got[2]).all()


def test_auto_keeps_the_ladder_under_a_forced_shape_and_picks_the_host_tail_otherwise(gm, oracle_mod, forced_options):
    import torch
    from conftest import random_scalars, rng_for
    g = gm.G1Jac("bn254")
    o = oracle_mod.Oracle("bn254", "g1")
    n = 1 << 12
    pts = o.gen_points(n, 99, 7, nthreads=8)
    sc = random_scalars(rng_for(77, n), g.curve, n)
    expected = o.msm_affine(pts, sc, nthreads=8)
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    forced_options(small_bits=1, glv=0)  # the sorted pipeline, not the fused small-n kernel
    assert gm.get_option("reduce_tail") == 0
    runs = plane_runs(gm)
    assert (g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n)) == expected).all()
    assert plane_runs(gm) == runs + 1, "auto did not select the host tail"
    c = g.default_window_bits(n)
    totals = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)  # window totals for a caller: the ladder, as ever
    assert plane_runs(gm) == runs + 1
    assert (g.jac_to_affine(g.fold_windows(totals, c)) == expected).all()
    forced_options(reduce_shape=2 | 2 << 4 | 2 << 6)  # log2L = 2, two levels, k_combine_we
    assert (g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n)) == expected).all()
    assert plane_runs(gm) == runs + 1, "a forced shape must run the ladder"
    forced_options(reduce_shape=0, reduce_tail=1)
    assert (g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n)) == expected).all()
    assert plane_runs(gm) == runs + 1


def test_other_groups_keep_the_ladder(gm, oracle_mod, forced_options):
    """a group without the plane kernels ignores the option"""
    import torch
    from conftest import random_scalars, rng_for
    g = gm.G1Jac("bls12_381")
    o = oracle_mod.Oracle("bls12_381", "g1")
    n = 1 << 11
    pts = o.gen_points(n, 5, 3, nthreads=8)
    sc = random_scalars(rng_for(78, n), g.curve, n)
    d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    forced_options(small_bits=1, glv=0, reduce_tail=2)
    runs = plane_runs(gm)
    got = g.jac_to_affine(g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n))
    assert (got == o.msm_affine(pts, sc, nthreads=8)).all() and plane_runs(gm) == runs
