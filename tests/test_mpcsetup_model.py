"""What gmsm_linear_combinations and gmsm_update_monomials are defined to compute, pinned to what the reference computes
(tests/mpcsetup_model.py), on subgroup points in Python integers - no GPU, no library."""
import importlib
import random

import pytest

import mpcsetup_model as mm

gm = importlib.import_module("gnark-crypto_amd")
GROUPS = [("bn254", "g1"), ("bls12_381", "g1"), ("bw6_761", "g1"), ("bn254", "g2")]
ENDS = [[2], [5], [2, 4], [3, 5, 9]]


@pytest.fixture(scope="module")
def cases(pyref_mod):
    """per group: the pyref Group and 12 points [k]Gen, two of them at infinity"""
    out = {}
    for gi, (curve, which) in enumerate(GROUPS):
        g = pyref_mod.Group(gm.CURVES[curve], which)
        rng = random.Random(0x3D0 + gi)
        pts = [g.mul(rng.randrange(1, 1 << 64), g.gen) for _ in range(12)]
        pts[1] = pts[6] = None
        out[(curve, which)] = (g, pts, rng.randrange(2, g.c.r))
    return out


@pytest.mark.parametrize("curve,which", GROUPS)
@pytest.mark.parametrize("ends", ENDS, ids=lambda e: "-".join(map(str, e)))
def test_route_of_the_reference_equals_the_definition(cases, curve, which, ends):
    g, pts, r = cases[(curve, which)]
    A = pts[:ends[-1]]
    assert mm.reference_linear_combinations(g, A, r, ends) == mm.direct_linear_combinations(g, A, r, ends)


@pytest.mark.parametrize("curve,which", GROUPS)
def test_shifted_is_truncated_over_r_shifted_for_a_geometric_slice(cases, curve, which):
    g, _, r = cases[(curve, which)]
    tau = 0x1234567
    A = [g.mul(pow(tau, i, g.c.r), g.gen) for i in range(6)]
    t, s = mm.direct_linear_combinations(g, A, r, [6])
    assert s == g.mul(tau, t)


@pytest.mark.parametrize("curve,which", GROUPS)
def test_update_monomials_loop_gives_the_powers(cases, curve, which):
    g, pts, r = cases[(curve, which)]
    for n in (2, 3, 7):
        A = pts[:n]
        assert mm.reference_update_monomials(g, A, r) == [g.mul(pow(r, i, g.c.r), P) if P is not None else None for i, P in enumerate(A)]


def test_refusals():
    for n, ends, text in ((4, [1, 4], "at least 2"), (4, [2, 3], "at least 2"), (5, [2, 4], "lengths mismatch"), (4, [4, 2], "at least 2")):
        with pytest.raises(ValueError, match=text):
            mm.check_ends(n, ends)
