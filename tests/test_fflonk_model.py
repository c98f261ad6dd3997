"""The shortcut of gmsm_fflonk.h is the reference's function (no GPU, no library): tests/fflonk_model.py restates
fflonk.BatchOpen as written (getNextDivisorRMinusOne, getIthRootOne, extendSet, Fold, eval at z^t, then shplonk.BatchOpen as
written on the folded polynomials and the extended sets) and the formulation the device runs (per-member chains,
interleaved accumulation, inner claimed values from the outer ones, L through the pack index); the two must agree on w
(trailing zeros stripped), on w' and on both sets of claimed values over the three scalar fields. Also pinned here:
NextDivisor(1..16) per field, the 100-trial limit, and the exact order of the t-th root of one."""
import itertools

import pytest

import fflonk_model as fm
import shplonk_model as sm
from conftest import rng_for

CURVES = ["bn254", "bls12_381", "bw6_761"]
DIVISORS = {"bn254": [1, 2, 3, 4, 6, 6, 8, 8, 9, 12, 12, 12, 13, 16, 16, 16],
            "bls12_381": [1, 2, 3, 4, 6, 6, 8, 8, 11, 11, 11, 12, 16, 16, 16, 16]}


def _rand(rng, r, count):
    return [int.from_bytes(rng.bytes(64), "little") % r for _ in range(count)]


def _agree(packs, points, gamma, z, r, g):
    w_ref, claimed_ref, folded_ref, wp_ref = fm.reference_batch_open(packs, points, gamma, z, r, g)
    w, claimed, folded, wp = fm.shortcut_batch_open(packs, points, gamma, z, r, g)
    ts = [fm.next_divisor(len(p), r) for p in packs]
    maxfold = max(t * max(len(q) for q in p) for p, t in zip(packs, ts))
    assert len(w) == maxfold and len(wp) == maxfold - 1
    assert sm.strip(w) == sm.strip(w_ref)
    assert claimed == claimed_ref and folded == folded_ref
    assert [len(rows) for rows in claimed] == ts and [len(v) for v in folded] == [t * len(s) for t, s in zip(ts, points)]
    assert wp + [0] * (len(wp_ref) - len(wp)) == wp_ref  # the reference's padding above the true degree is zero


@pytest.mark.parametrize("curve", CURVES)
def test_next_divisor_is_pinned(gm, curve):
    r = gm.CURVES[curve].r
    got = [fm.next_divisor(n, r) for n in range(1, 17)]
    if curve in DIVISORS:
        assert got == DIVISORS[curve]
    # from the modulus alone (BW6-761: nothing typed in): the smallest divisor of r - 1 at or above n
    assert got == [next(t for t in range(n, n + 100) if (r - 1) % t == 0) for n in range(1, 17)]
    assert all(t >= n and (r - 1) % t == 0 for n, t in zip(range(1, 17), got))


@pytest.mark.parametrize("curve", CURVES)
def test_next_divisor_gives_up_after_100_trials(gm, curve):
    r = gm.CURVES[curve].r
    n = next(n for n in itertools.count(1 << 20) if all((r - 1) % t for t in range(n, n + 101)))
    assert fm.next_divisor(n, r) is None
    # a divisor exactly 100 steps away is met as the counter reaches zero: the reference panics there too
    d = next(t for t in itertools.count(1 << 20) if (r - 1) % t == 0 and all((r - 1) % u for u in range(t - 100, t)))
    assert fm.next_divisor(d - 100, r) is None and fm.next_divisor(d - 99, r) == d


@pytest.mark.parametrize("curve", CURVES)
def test_root_of_one_has_exact_order(gm, curve):
    c = gm.CURVES[curve]
    for t in sorted({fm.next_divisor(n, c.r) for n in range(1, 17)}):
        w = fm.ith_root_one(t, c.r, c.fr_mult_gen)
        assert pow(w, t, c.r) == 1
        assert all(pow(w, t // q, c.r) != 1 for q in range(2, t + 1) if t % q == 0)  # no proper divisor of t is the order
        ext = fm.extend_set([3, 5], t, c.r, c.fr_mult_gen)
        assert len(set(ext)) == 2 * t and all(pow(x, t, c.r) == pow(b, t, c.r) for i, b in enumerate((3, 5)) for x in ext[i * t:(i + 1) * t])


def test_fold_interleaves():
    r = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # BN254: 5 polynomials take t = 6
    assert fm.fold([[1, 2], [3], [], [4, 5, 6], [7]], r) == [1, 3, 0, 4, 7, 0, 2, 0, 0, 5, 0, 0, 0, 0, 0, 6, 0, 0]
    assert fm.fold([[9, 8, 7]], r) == [9, 8, 7]


@pytest.mark.parametrize("curve", CURVES)
def test_one_pack_every_small_shape(gm, curve):
    c = gm.CURVES[curve]
    r, g = c.r, c.fr_mult_gen
    rng = rng_for(0xFF10, CURVES.index(curve))
    gamma, z = _rand(rng, r, 2)
    pool = [1] + _rand(rng, r, 3)  # 1 and r - 1 share an orbit for even t: refused, not modelled
    coeffs = _rand(rng, r, 40)
    # 1, 2, 3 and 5 members (t = 1, 2, 3 and 6 - padded slots - on the pinned fields), lengths that end a chain early, an empty member
    for lens in ((1,), (4,), (1, 1), (3, 5), (5, 0), (2, 4, 1), (0, 3, 3), (6, 2, 0, 3, 1)):
        for m in (1, 2, 3):
            order = list(rng.permutation(len(pool)))
            pack = [coeffs[8 * j:8 * j + n] for j, n in enumerate(lens)]
            _agree([pack], [[pool[i] for i in order[:m]]], gamma, z, r, g)
    _agree([[coeffs[:2]]], [[0, 1, pool[2]]], gamma, z, r, g)  # z = 0 is legal with t = 1


@pytest.mark.parametrize("curve", CURVES)
def test_several_packs_and_edge_challenges(gm, curve):
    c = gm.CURVES[curve]
    r, g = c.r, c.fr_mult_gen
    rng = rng_for(0xFF11, CURVES.index(curve))
    ra, rb, rc, rd = _rand(rng, r, 4)
    packs = [[_rand(rng, r, n) for n in lens] for lens in ((3, 9, 1), (7, 2, 0, 5, 4), (2,), (1, 1))]
    points = [[ra, 1], [r - 1], [0, 1, rb], [rc, rd]]  # the point 1 sits in two packs
    for gamma, z in ((_rand(rng, r, 1)[0], _rand(rng, r, 1)[0]), (0, 0), (1, r - 1), (_rand(rng, r, 1)[0], ra)):
        _agree(packs, points, gamma, z, r, g)  # the last z is a root of Z_T: L and w' are still defined
    _agree(packs[:2], points[:2], ra, rb, r, g)
    _agree(packs[3:], points[3:], ra, rb, r, g)  # every chain runs out: w = 0
