"""The model and the cases of tests/frontend_cases.py, on the host: recode() against the reference's partitionScalars
(oracle.partition_scalars) for the widths it has, its round trip for the wider ones; and, for layouts of 256 and 64 compute
units (gmsm_debug_run_layout: host arithmetic only), that every named case meets the condition it is named for at the sizes
tests/test_gpu_frontend_shapes.py runs it at, and that the unforced shapes of that file select what they are listed for. The
conditions are recomputed from the bucket populations and the layout's integers alone: when a tuning constant of the pipeline
moves and a case no longer reaches its regime, this file fails (a case that cannot be built raises CaseDoesNotFit)."""
import random

import numpy as np
import pytest

import frontend_cases as fc

GROUPS = [("bn254", "g1"), ("bn254", "g2"), ("bw6_761", "g1")]
CUS = (256, 64)


def _group(gm, curve, which):
    return (gm.G1Jac if which == "g1" else gm.G2Jac)(curve)


def _edge_scalars(curve):
    r = curve.r
    return [0, 1, 2, r - 1, r - 2, (1 << 16) - 1, 1 << 16, 1 << 15, (1 << 15) - 1, (1 << 64) - 1, 1 << 64, (1 << 128) + 12345, r >> 1]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bw6_761"])
def test_recode_is_partition_scalars(gm, oracle_mod, curve):
    g = _group(gm, curve, "g1")
    o = oracle_mod.Oracle(curve, "g1")
    cv = g.curve
    rng = random.Random(f"recode/{curve}")
    vals = _edge_scalars(cv) + [rng.randrange(cv.r) for _ in range(200)]
    sc = fc.mont_limbs(cv, vals)
    assert fc.ints_from_mont(cv, sc) == vals
    for c in range(2, 17):
        assert o.nb_chunks(c) == fc.num_windows(cv.fr_bits, c)
        want = o.partition_scalars(sc, c).astype(np.int64)
        got = np.array([[fc.code(d) for d in fc.recode(cv, v, c)] for v in vals], dtype=np.int64).T
        assert (got == want).all(), c
        D = fc.recode_array(cv, vals, c)
        assert (np.where(D > 0, 2 * D, np.where(D < 0, 2 * (-D - 1) + 1, 0)) == want).all(), c
        assert fc.nbuckets(cv.fr_bits, c) > np.max(np.abs(D)) - 1


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bw6_761"])
def test_recode_round_trip_at_the_wide_widths(gm, curve):
    cv = _group(gm, curve, "g1").curve
    rng = random.Random(f"wide/{curve}")
    vals = _edge_scalars(cv) + [rng.randrange(cv.r) for _ in range(200)]
    for c in range(17, 25):
        nwin, half = fc.num_windows(cv.fr_bits, c), 1 << (c - 1)
        D = fc.recode_array(cv, vals, c)
        for i, v in enumerate(vals):
            ds = fc.recode(cv, v, c)
            assert len(ds) == nwin and list(D[:, i]) == ds
            assert all(-half <= d < half for d in ds[:-1]) and 0 <= ds[-1] <= (cv.r >> (c * (nwin - 1))) + 1
            assert fc.scalar_from_digits(cv, ds, c) == v
            assert all(abs(d) - 1 < fc.nbuckets(cv.fr_bits, c) for d in ds)
        assert fc.scalars_from_digit_matrix(cv, D, c) == vals


def test_the_constants_are_the_headers(gm):
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(gm.__file__)), "csrc", "gmsm_kernels.h")).read()
    for name in ("PART_CHUNK", "HEAVY_SUB", "FIXUP_MAXWALK", "LONG_PIECE"):
        m = re.search(r"constexpr uint32_t " + name + r" = (\d+)", src)
        assert m and int(m.group(1)) == getattr(fc, name), name


# the sizes and widths the device file runs the cases at (shared with it)
@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("curve,which", GROUPS)
def test_chains_and_gaps_meet_their_conditions(gm, curve, which, cus):
    g = _group(gm, curve, which)
    for name, check in (("chains", fc.check_chains), ("gaps", fc.check_gaps)):
        L, pops = fc.fit(gm, g.gid, cus, name, fc.CASE_C[curve], fc.CASE_SIZES)
        check(L, pops[0])
        print(name, curve, which, cus, {k: L[k] for k in ("n_points", "c", "seg", "fbits", "nparts", "stage_cap")})
        assert list(pops) == [0] and len(pops[0]) == L["NB"] == fc.nbuckets(g.curve.fr_bits, L["c"])
        for w in fc.case_windows(L):
            D = fc.case_digits(g.curve, L, pops, w, name)
            assert (fc.bucket_populations(D, L["NB"])[w] == np.asarray(pops[0])).all() and not D[-1].any()
            if name == "chains":
                for content in fc.CONTENTS:
                    bases, d = fc.chain_contents(g.curve, L, pops[0], D[w], content, 3, 5)
                    assert (fc.bucket_populations(d[None, :], L["NB"])[0] == np.asarray(pops[0])).all()
                    heads = [i for i, how in bases.changed.items() if how[0] != "inf"]
                    assert all(abs(d[i]) == abs(d[bases.changed[i][1]]) for i in heads)  # copies stay in their base's bucket
                    assert (content in ("repeated", "plus_minus")) == bool(heads)


@pytest.mark.parametrize("cus", CUS)
def test_stage_exact_and_heavy_rows_meet_their_conditions(gm, cus):
    g = _group(gm, "bn254", "g1")
    for variant in ("spread", "one"):
        L, pops = fc.fit(gm, g.gid, cus, "stage_exact", fc.SORT_C, fc.SORT_SIZES, variant=variant)
        fc.check_stage_exact(L, pops[0], variant)
    L, pops = fc.fit(gm, g.gid, cus, "heavy_rows", fc.SORT_C, fc.SORT_SIZES)
    for w in fc.case_windows(L):
        D = fc.case_digits(g.curve, L, pops, w, "heavy_rows")
        fc.check_heavy_rows(L, fc.bucket_populations(D, L["NB"]), w)


@pytest.mark.parametrize("cus", CUS)
def test_the_shared_bucket_set_meets_the_chains_conditions(gm, cus):
    g = _group(gm, "bn254", "g1")
    L, pops = fc.fit(gm, g.gid, cus, "chains", fc.CASE_C["bn254"], fc.CASE_SIZES, shared=1)
    fc.check_shared_chains(L, pops[0])
    D = fc.shared_digits(g.curve, L, pops[0])
    assert not D[-1].any() and (D >= 0).all()


def test_a_case_that_cannot_be_built_raises(gm):
    g = _group(gm, "bn254", "g1")
    with pytest.raises(fc.CaseDoesNotFit):   # 1025 points cannot hold chains of 513 links
        fc.fit(gm, g.gid, 256, "chains", 12, [1025])
    with pytest.raises(fc.CaseDoesNotFit):   # 2^16 buckets on 2^13 points: fbits is clamped, one partition
        fc.fit(gm, g.gid, 256, "stage_exact", 17, [1 << 13], variant="spread")
    with pytest.raises(fc.CaseDoesNotFit):   # c = 2 on BN254: the top window widens the bucket set
        fc.fit(gm, g.gid, 256, "gaps", 2, [4096])


@pytest.mark.parametrize("cus", CUS)
def test_the_table_of_unforced_shapes_is_what_it_says(gm, cus):
    g = _group(gm, "bn254", "g1")
    assert len(fc.UNFORCED) == 14
    for (n, c) in fc.UNFORCED:
        fc.check_unforced(fc.layout(gm, g.gid, cus, n, c))
    # and the conditions bite: a neighbouring shape fails each
    for (n, c), (n2, c2) in (((12288, 13), (12296, 13)), ((12289, 13), (12290, 13)), ((65541, 17), (65544, 17)), ((1 << 16, 4), (1 << 16, 6)),
                             ((1 << 17, 20), (1 << 15, 20))):
        L = fc.layout(gm, g.gid, cus, n2, c2)
        assert not fc.UNFORCED[(n, c)][1](L), (n2, c2)


@pytest.mark.parametrize("content", fc.CONTENTS)
@pytest.mark.parametrize("curve,which", GROUPS[:2])
def test_expected_totals_are_the_references_bucket_sums(gm, oracle_mod, curve, which, content):
    """[sum_i a_i d_w(s_i)]G against the reference's processChunk over the same bases and digits: the changed bases (infinity,
    copies, negatives) and the linear form of the weighted sum, once per content"""
    g = _group(gm, curve, which)
    o = oracle_mod.Oracle(curve, which)
    L, pops = fc.fit(gm, g.gid, 256, "chains", fc.CASE_C[curve], fc.CASE_SIZES)
    w = fc.case_windows(L)[1]
    D = fc.case_digits(g.curve, L, pops, w, "chains")
    bases, D[w] = fc.chain_contents(g.curve, L, pops[0], D[w], content, 3, 5)
    vals = fc.scalars_from_digit_matrix(g.curve, D, L["c"])
    codes = o.partition_scalars(fc.mont_limbs(g.curve, vals), L["c"])
    pts = bases.points(o)
    assert [bases.weighted(D[k]) for k in (0, w)] == [bases.weighted_ints([int(v) for v in D[k]]) for k in (0, w)]
    totals = [o.process_chunk(L["c"], pts, codes[k]) for k in (0, w, L["nwd"] - 1)]
    fc.check_totals(o, totals, [fc.expected_affine(o, bases.weighted(D[k])) for k in (0, w, L["nwd"] - 1)], content)
