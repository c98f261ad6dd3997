"""The stages between the digits and the buckets of the sorted MultiExp pipeline - the sort (k_decompose*, k_part_hist / colscan /
rowscan / scatter, k_fine_sort, k_heavy_hist / scan / place), the accumulation (k_accumulate_seg) and the split-bucket fix-up
(k_fixup_seg, k_fixup_seg_q, k_fixup_bucket, k_fixup_long) - at the geometry edges the end-to-end parity tests do not select.
tests/frontend_cases.py builds the inputs and says what each case is; tests/test_frontend_cases_model.py shows on the host that
each reaches its regime. Here every window total of window_sums_device must equal the model's [sum_i a_i d_w(s_i)]G limb for limb
(the oracle's scalar multiplication and conversions; no group arithmetic of this library on the expected side), under
glv = 0, tables = 0, with the layout taken for the device's own CU count:

(a) seeded uniform scalars on BN254 G1 (the sort kernels are not templated on the group) at the n and c of frontend_cases.UNFORCED:
    chunk boundaries and alignment of k_part_hist / k_part_scatter for 16- and 32-bit codes, fbits = 0, fbits + lidx = 32;
(b) the named cases: stage_exact and heavy_rows on BN254 G1; chains with its four contents and gaps on BN254 G1 (k_fixup_seg),
    BN254 G2 (k_fixup_seg_q over Fp2) and BW6-761 G1 (k_fixup_seg_q over the 28-limb field); the case window is once window 0 and
    once a middle one, the other windows hold uniform non-zero digits;
(c) the chains populations in the shared bucket set of window tables (k_fixup_bucket), by value: [sum a_i s_i]G.
The last test prints the layouts the device gave (pytest -s)."""
import numpy as np
import pytest

import frontend_cases as fc

pytestmark = pytest.mark.gpu

K0, K1 = 0x5EED0FBA5E5, 0x9E3779B97F4A7C15   # base i = [K0 + i K1]G
GROUPS = [("bn254", "g1"), ("bn254", "g2"), ("bw6_761", "g1")]
LAYOUTS = {}  # (case, group) -> the layout integers the description of a run quotes


@pytest.fixture(autouse=True)
def plain_sorted_pipeline(gm):
    with gm.options(glv=0, tables=0):
        yield


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count  # what gmsm_context.h reads


def groups(gm, oracle_mod, curve, which):
    return (gm.G1Jac if which == "g1" else gm.G2Jac)(curve), oracle_mod.Oracle(curve, which)


def small_runs(gm):
    return int(gm._lib.load().gmsm_debug_small_runs())


def note(case, curve, which, L):
    LAYOUTS[(case, curve, which)] = {k: L[k] for k in ("n_points", "c", "seg", "fbits", "nparts", "stage_cap", "tpw", "lidx", "pchunks", "d16")}


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def window_totals_match(gm, g, o, L, bases, vals, D, tag):
    """every window total of the run against the model"""
    n, c = L["n_points"], L["c"]
    assert D.shape == (g.num_windows(c), n) == (L["nwd"], n)
    d_pts, d_sc = to_device(bases.points(o)), to_device(fc.mont_limbs(g.curve, vals))
    small = small_runs(gm)
    totals = g.window_sums_device(d_pts.data_ptr(), d_sc.data_ptr(), n, c)
    assert small_runs(gm) == small, "the fused small-n kernel took the call"
    want = [fc.expected_affine(o, bases.weighted(D[w])) for w in range(D.shape[0])]
    fc.check_totals(o, totals, want, tag)


# ------------------------------------------------------------------ (a) the sort geometry under uniform scalars
@pytest.mark.parametrize("n,c", sorted(fc.UNFORCED))
def test_sort_geometry_under_uniform_scalars(gm, oracle_mod, n, c):
    g, o = groups(gm, oracle_mod, "bn254", "g1")
    L = fc.layout(gm, g.gid, device_cus(), n, c)
    fc.check_unforced(L)
    note(f"uniform n={n} c={c}", "bn254", "g1", L)
    vals = fc.uniform_scalars(g.curve, n, c)
    vals[11] = 0
    D = fc.recode_array(g.curve, vals, c)
    bases = fc.Bases(g.curve, n, K0, K1, {i: ("inf",) for i in (5, n // 3, n - 2)})
    window_totals_match(gm, g, o, L, bases, vals, D, (n, c))


# ------------------------------------------------------------------ (b) the named cases
def run_case(gm, oracle_mod, curve, which, name, c, sizes, window, variant=None, content="distinct"):
    g, o = groups(gm, oracle_mod, curve, which)
    L, pops = fc.fit(gm, g.gid, device_cus(), name, c, sizes, variant=variant)
    w = fc.case_windows(L)[window]
    D = fc.case_digits(g.curve, L, pops, w, name, variant)
    allpops = fc.bucket_populations(D, L["NB"])
    if name == "chains":
        fc.check_chains(L, allpops[w])
    elif name == "gaps":
        fc.check_gaps(L, allpops[w])
    elif name == "stage_exact":
        fc.check_stage_exact(L, allpops[w], variant)
    else:
        fc.check_heavy_rows(L, allpops, w)
    note(name, curve, which, L)
    bases = fc.Bases(g.curve, L["n_points"], K0, K1)
    if name == "chains":
        bases, D[w] = fc.chain_contents(g.curve, L, pops[0], D[w], content, K0, K1)
        assert (fc.bucket_populations(D, L["NB"]) == allpops).all()
    vals = fc.scalars_from_digit_matrix(g.curve, D, L["c"])
    window_totals_match(gm, g, o, L, bases, vals, D, (name, variant, content, curve, which, w))


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("variant", ["spread", "one"])
def test_stage_exact(gm, oracle_mod, variant, window):
    run_case(gm, oracle_mod, "bn254", "g1", "stage_exact", fc.SORT_C, fc.SORT_SIZES, window, variant=variant)


@pytest.mark.parametrize("window", [0, 1])
def test_heavy_rows(gm, oracle_mod, window):
    run_case(gm, oracle_mod, "bn254", "g1", "heavy_rows", fc.SORT_C, fc.SORT_SIZES, window)


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("content", fc.CONTENTS)
@pytest.mark.parametrize("curve,which", GROUPS)
def test_chains(gm, oracle_mod, curve, which, content, window):
    run_case(gm, oracle_mod, curve, which, "chains", fc.CASE_C[curve], fc.CASE_SIZES, window, content=content)


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("curve,which", GROUPS)
def test_gaps(gm, oracle_mod, curve, which, window):
    run_case(gm, oracle_mod, curve, which, "gaps", fc.CASE_C[curve], fc.CASE_SIZES, window)


# ------------------------------------------------------------------ (c) the per-bucket fix-up of the shared bucket set
def test_chains_in_the_shared_bucket_set_of_window_tables(gm, oracle_mod, forced_options):
    g, o = groups(gm, oracle_mod, "bn254", "g1")
    c = fc.CASE_C["bn254"]
    forced_options(glv=0, small_bits=1, window_bits=c)
    L, pops = fc.fit(gm, g.gid, device_cus(), "chains", c, fc.CASE_SIZES, shared=1)
    fc.check_shared_chains(L, pops[0])
    note("chains, shared set", "bn254", "g1", L)
    n = L["n_points"]
    vals = fc.scalars_from_digit_matrix(g.curve, fc.shared_digits(g.curve, L, pops[0]), c)
    bases = fc.Bases(g.curve, n, K0, K1)
    want = fc.expected_affine(o, bases.weighted_ints(vals))
    d_sc = to_device(fc.mont_limbs(g.curve, vals))
    rb = g.register_bases(points=bases.points(o))
    try:
        assert rb.precompute(c) == c
        runs = int(gm._lib.load().gmsm_debug_table_runs())
        with gm.options(tables=2):
            got = g.jac_to_affine(rb.multiexp_device(d_sc.data_ptr(), n))
        assert int(gm._lib.load().gmsm_debug_table_runs()) == runs + 1
        assert want is not None and (got == want).all()
    finally:
        rb.release()


def test_options_are_back_and_layouts_are_listed(gm):
    assert gm.get_option("window_bits") == 0
    for key, L in sorted(LAYOUTS.items()):
        print(*key, L)
