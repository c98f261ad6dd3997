"""The cases of tests/point_batch_cases.py, on the host: every constructed input has the property it is named for - the borrow
chains and the doubled top bucket set of the fixed-base digits (against frontend_cases.recode, the partitionScalars model), the
GLV pairs (against GlvParams.split, which test_glv_split_on_the_device ties the device to), the groups at infinity, and more
workgroups in a sumcheck round than k_gkr_finish has lanes. The constants the cases are sized by are read back from the sources:
when SCALE_CHUNK, K, GKR_TPB or FRI_TPB move, this file fails first and names what has to move with them."""
import os
import re
import warnings

import pytest

import frontend_cases as fc
import point_batch_cases as pc

CURVES = ["bn254", "bls12_381", "bw6_761"]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnark-crypto_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_constants_are_the_sources():
    assert re.search(r"SCALE_CHUNK = \(size_t\)1 << (\d+);", _source("gmsm_scale.h")).group(1) == str(pc.SCALE_CHUNK.bit_length() - 1), \
        "SCALE_CHUNK moved: the second-chunk sizes of test_gpu_point_batches.py move with it"
    norm = re.search(r"static int normalize_records\(.*?\n    }\n", _source("gmsm_group.h"), re.S).group(0)
    assert "constexpr int K = %d;" % pc.NORMALIZE_K in norm and "dim3(%d)" % pc.NORMALIZE_TPB in norm, \
        "K or the workgroup of k_batch_normalize moved: NORMALIZE_SIZES and infinity_masks move with them"
    expr = _source("gmsm_iop_expr.h")
    assert "constexpr unsigned EXPR_TPB = %d;" % pc.EXPR_TPB in expr and "EXPR_LDS_BYTES = 64 * 1024;" in expr
    assert "constexpr unsigned GKR_TPB = EXPR_TPB;" in _source("gmsm_gkr.h"), "GKR_TPB moved: MANY_WORKGROUPS of test_gpu_gkr.py moves with it"
    assert "constexpr unsigned FRI_TPB = %d;" % pc.FRI_TPB in _source("gmsm_fri.h"), "FRI_TPB moved: test_fold_across_workgroups moves with it"
    assert pc.EXPR_LDS_BYTES == 64 * 1024


# ------------------------------------------------------------------ fixed base
@pytest.mark.parametrize("curve", CURVES)
def test_borrow_cases_have_their_digits(gm, curve):
    cv = gm.CURVES[curve]
    for c in pc.FIXED_BASE_WIDTHS:
        nwin, half = fc.num_windows(cv.fr_bits, c), 1 << (c - 1)
        cases = pc.borrow_cases(cv, c)
        assert cases == pc.borrow_cases(curve, c)  # by name too
        names = [name for name, _, _ in cases]
        assert len(set(names)) == len(names) and {"all_half", "all_half_minus_one", "ones_zero", "zero_ones", "half_zero", "r_minus_1",
                                                  "r_minus_2", "top_max"} <= set(names)
        assert any(n.startswith("2^") for n in names) and any(n.startswith("below_2^") for n in names)
        for name, s, digits in cases:
            got = fc.recode(cv, s, c)
            assert 0 <= s < cv.r and len(got) == nwin and sum(d << (c * w) for w, d in enumerate(got)) == s, (c, name)
            assert all(-half <= d < half for d in got[:-1]) and got[-1] >= 0, (c, name)
            if digits is not None:
                assert got == digits, (c, name)
            # the borrow out of window w, from the bits alone: the digit is the window plus the carry in, minus 2^c when it borrows
            carry = 0
            for w in range(nwin - 1):
                raw = (s >> (c * w)) & ((1 << c) - 1)
                borrows = raw + carry >= half
                assert (got[w] < 0 or (got[w] == 0 and raw + carry == 1 << c)) == borrows, (c, name, w)
                carry = 1 if borrows else 0
            if name == "all_half":
                assert all(d < 0 for d in got[:-1]) and got[-1] == ((cv.r - 1) >> (c * (nwin - 1))), (c, name)  # the longest chain
            if name == "all_half_minus_one":
                assert all(d == half - 1 for d in got[:-1]), (c, name)  # no borrow anywhere
            if name == "top_max":
                assert got[-1] == (cv.r - 1) >> (c * (nwin - 1)) and s + (1 << (c * (nwin - 1))) >= cv.r, (c, name)
        assert cases[[n for n, _, _ in cases].index("r_minus_1")][1] == cv.r - 1
        assert pc.borrow_scalars(cv, c) == [s for _, s, _ in cases]


def test_a_window_boundary_meets_a_word_edge_at_every_width(gm):
    seen = set()
    for curve in CURVES:
        cv = gm.CURVES[curve]
        for c in pc.FIXED_BASE_WIDTHS:
            edges = pc.word_edges(cv, c)
            assert edges, (curve, c)
            assert all((c * j) % 32 == res and 2 ** (c * j) < cv.r for j, res in edges)
            seen |= {res for _, res in edges}
    assert seen == {31, 0, 1}
    with pytest.raises(pc.CaseCannotBeBuilt):  # what cannot be built raises: no boundary of 13-bit windows of a 48-bit scalar is near a word edge
        class Tiny:
            name, r, fr_bits = "tiny", (1 << 48) - 59, 48
        pc.borrow_cases(Tiny, 13)


@pytest.mark.parametrize("curve,c", pc.EXACTLY_DIVIDING)
def test_the_doubled_top_bucket_set_is_entered(gm, curve, c):
    cv = gm.CURVES[curve]
    assert cv.fr_bits % c == 0 and fc.nbuckets(cv.fr_bits, c) == 1 << c  # lastC = c + 1
    tops = [fc.recode(cv, s, c)[-1] - 1 for s in pc.borrow_scalars(cv, c)]  # the top window's bucket index (-1: the digit 0)
    assert max(tops) < 1 << c and max(tops) >= 1 << (c - 1), tops
    assert sum(1 for t in tops if t >= 1 << (c - 1)) >= 2
    groups = {(cu, w) for cu, w, cc in pc.FIXED_BASE_CASES if (cu, cc) == (curve, c)}
    assert groups, "no device case runs this width"


def test_the_fixed_base_cases_are_the_listed_ones():
    assert {c for cu, w, c in pc.FIXED_BASE_CASES if (cu, w) == ("bn254", "g1")} == set(range(2, 15))
    assert {(cu, w) for cu, w, _ in pc.FIXED_BASE_CASES} == {(cu, w) for cu in CURVES for w in ("g1", "g2")}
    assert len(set(pc.FIXED_BASE_CASES)) == len(pc.FIXED_BASE_CASES) == 13 + 11


# ------------------------------------------------------------------ the GLV walk
@pytest.mark.parametrize("curve", CURVES)
def test_glv_pattern_pairs_are_what_the_split_returns(gm, curve):
    cv = gm.CURVES[curve]
    glv = gm.curves.GlvParams(cv)
    assert glv.a[0] > 0 and glv.a[1] > 0  # a11, a21: with e1, e2 >= 0 no half k1 is negative, and k1 = 0 only for s = 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pc._glv_cache.pop(curve, None)
        cases = pc.glv_pattern_cases(curve)
    assert cases == pc.glv_pattern_cases(cv)
    assert any("another representative" in str(w.message) for w in caught)  # the dropped pairs are reported
    reached = {}
    for name, k1, k2, s in cases:
        assert 0 <= s < cv.r and (k1 + k2 * glv.lam - s) % cv.r == 0 and glv.split(s) == (k1, k2), name
        assert abs(k1) < 1 << glv.bits and abs(k2) < 1 << glv.bits
        reached.setdefault(pc.glv_kind(k1, k2), set()).add(pc.glv_signs(k1, k2))
    # in both directions: every kind listed is met, and a kind that is not listed has become reachable - extend the list
    assert reached == pc.GLV_REACHABLE[curve], reached
    assert pc.glv_pattern_scalars(cv) == [s for _, _, _, s in cases]
    assert {cv.r - 1, cv.r - glv.lam, (1 - glv.lam) % cv.r} <= set(pc.glv_pattern_scalars(cv))
    # the search does not decide what is reachable: the edge scalars and 20000 uniform ones show nothing outside the table
    import random
    rng = random.Random("glv-reachable/" + curve)
    for s in pc.glv_edge_scalars(cv, glv.lam) + [rng.randrange(cv.r) for _ in range(20000)]:
        k1, k2 = glv.split(s)
        assert k1 > 0 and pc.glv_signs(k1, k2) in pc.GLV_REACHABLE[curve].get(pc.glv_kind(k1, k2), ()), hex(s)
    # not only a unit half: a walk over T[1] alone for (nearly) all of its GLV_BITS steps, over T[3] alone for more than two words
    # of them (the longest pair (t, +-t) the split returns on BW6-761 has 148 of 190 bits)
    for kind, least in (("only_T1", glv.bits - 2), ("only_T3", 65)):
        if kind in pc.GLV_REACHABLE[curve]:
            assert max(max(abs(k1), abs(k2)).bit_length() for _, k1, k2, _ in cases if pc.glv_kind(k1, k2) == kind) >= least, kind
    assert (1, 0, 1) in [(k1, k2, s) for _, k1, k2, s in cases]


# ------------------------------------------------------------------ normalisation
def test_infinity_masks_cover_every_pattern_in_every_group():
    K = pc.NORMALIZE_K
    assert set(pc.NORMALIZE_SIZES_WIDE) <= set(pc.NORMALIZE_SIZES) and {K - 1, K, K + 1, 64 * K - 1, 64 * K, 64 * K + 1} <= set(pc.NORMALIZE_SIZES)
    for n in pc.NORMALIZE_SIZES:
        masks = pc.infinity_masks(n)
        assert all(len(m) == n for _, m in masks) and masks[-1][1] == [True] * n
        groups = (n + K - 1) // K
        for g in range(groups):
            size = min(K, n - g * K)
            seen = {tuple(m[g * K:g * K + size]) for _, m in masks[:-1]}
            want = {tuple(pc._group_mask(p, size)) for p in pc.GROUP_PATTERNS}
            assert seen == want, (n, g)
            assert (True,) * size in seen and (False,) * size in seen  # the inversion of an untouched one; a group without infinities
        if n >= 2 * K:
            assert any(all(m[K:2 * K]) and not all(m[:K]) for _, m in masks)   # all of [32, 64)
            assert any(all(m[:K]) and not any(m[K + 1:2 * K - 1]) for _, m in masks)  # all of [0, 32)
            assert any(sum(m[K:2 * K]) == K - 1 for _, m in masks)          # every record but one


# ------------------------------------------------------------------ the sumcheck round
def test_round_lanes_is_the_host_code():
    assert pc.expr_lanes_for(32, 17) == 64 and pc.expr_lanes_for(32, 4) == 256 and pc.expr_lanes_for(48, 17) == 64  # gmsm_iop_expr.h's examples
    assert pc.round_lanes(32, 3, 1 << 17) == 256 and pc.round_lanes(32, 3, 128) == 128 and pc.round_lanes(32, 3, 1) == 64
    assert pc.round_lanes(48, 9, 1 << 15) == 128 and pc.round_lanes(48, 10, 1 << 15) == 64


def test_the_large_claims_have_more_workgroups_than_the_finish_has_lanes(gm):
    MANY_WORKGROUPS = pc.MANY_WORKGROUPS
    assert {(c, g) for c, g, _, _, _ in MANY_WORKGROUPS} == {("bw6_761", "pairs8"), ("bn254", "identity")}
    assert sorted(k for c, _, _, k, _ in MANY_WORKGROUPS if c == "bw6_761") == [1, 2]
    for curve, name, n, k, lanes in MANY_WORKGROUPS:
        cv = gm.CURVES[curve]
        f, m, degree = pc.GKR_GATES[name]
        code = gm.gkr.Gate(f, degree).code(curve, m)
        nregs = 1 + max((int(w) >> 8) & 0xFF for w in code.words)
        if name == "pairs8":
            assert nregs >= 10
        elem = 8 * cv.fr_limbs
        assert pc.round_lanes(elem, nregs, 1 << (n - 1)) == lanes
        blocks = pc.round_workgroups(elem, nregs, n)
        assert blocks[0] == 512 > pc.EXPR_TPB                      # the strided loop of k_gkr_finish takes a second step
        assert blocks[1] == pc.EXPR_TPB                            # exactly one
        assert blocks == sorted(blocks, reverse=True) and 2 in blocks and blocks[-1] == 1  # down to the single-workgroup shortcut
        stride = 1 << n
        assert max(blocks) <= (stride // 2 + 63) // 64             # the rows gkr_new sizes `partials` for suffice
