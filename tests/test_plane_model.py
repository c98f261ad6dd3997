"""The plane identity of the reduction's host tail and the Horner walk that applies its weights, over the integers mod a
prime (tests/plane_model.py, the step machines of k_combine_we<PLANES>, k_plane_sums and GroupHost::fold_planes):
    sum W_t + L sum_t t S_t  ==  fold_planes(plane sums),
for T pairs per window in 1, 63, 64, 65, 130, 4096 and 8192 (128 blocks, the most k_plane_sums takes), L in 2, 8, random and all-zero S_t, one and several windows, and the
workgroup sizes k_plane_sums is launched with (16 to 64 quads per plane)."""
import random

import pytest

import plane_model as pm
from combine_model import Group

R = (1 << 61) - 1  # a prime: Z_r, where a vanishing sum is infinity
TS = (1, 63, 64, 65, 130, 4096, 8192)


def pairs(rng, T, zero_S):
    S = [None if zero_S else rng.randrange(1, R) for _ in range(T)]
    W = [rng.randrange(1, R) if rng.randrange(5) else None for _ in range(T)]
    return S, W


def direct(S, W, L):
    v = (sum(w or 0 for w in W) + L * sum(t * (s or 0) for t, s in enumerate(S))) % R
    return v or None


def quads_for(T):
    H = (-(-T // pm.N) - 1).bit_length()
    return min(64, max(16, (1 << H) // 2))  # Pipeline::enqueue_reduce_kernels


@pytest.mark.parametrize("zero_S", [False, True])
@pytest.mark.parametrize("log2L", [1, 3])
@pytest.mark.parametrize("T", TS)
def test_one_window(T, log2L, zero_S):
    rng = random.Random(f"planes/{T}/{log2L}/{zero_S}")
    grp = Group(R)
    S, W = pairs(rng, T, zero_S)
    planes = pm.window_planes(S, W, grp, quads_for(T))
    assert len(planes) == 7 + (-(-T // 64) - 1).bit_length()
    got, dbls, adds = pm.fold_planes([planes], 16, log2L, grp)
    assert got == direct(S, W, 1 << log2L)
    assert adds == sum(p is not None for p in planes) and dbls <= log2L + len(planes) - 2
    if zero_S:
        assert all(p is None for p in planes[1:])


@pytest.mark.parametrize("nq", [16, 32, 64])
def test_passes_of_a_small_workgroup_give_the_same_sums(nq):
    """fewer quads than additions in a step: the passes of one step are independent"""
    rng = random.Random(f"planes/passes/{nq}")
    S, W = pairs(rng, 4096, False)
    grp = Group(R)
    assert pm.window_planes(S, W, grp, nq) == pm.window_planes(S, W, grp, 128)


@pytest.mark.parametrize("T,log2L,c", [(4096, 3, 16), (65, 1, 8), (130, 3, 13), (64, 1, 7), (4096, 3, 12)])
def test_horner_walk_over_windows(T, log2L, c):
    """MSM = sum_w 2^(c w) total_w; with c below log2L + 6 + H the planes of neighbouring windows share bit positions"""
    rng = random.Random(f"planes/windows/{T}/{log2L}/{c}")
    grp = Group(R)
    nwin = 5
    planes, want = [], 0
    for w in range(nwin):
        zero = w == 2  # a window with no finite plane at all
        S, W = pairs(rng, T, zero)
        if zero:
            W = [None] * T
        planes.append(pm.window_planes(S, W, grp, quads_for(T)))
        want += (direct(S, W, 1 << log2L) or 0) << (c * w)
    assert all(p is None for p in planes[2])
    got, dbls, adds = pm.fold_planes(planes, c, log2L, grp)
    assert got == (want % R or None)
    assert dbls <= c * (nwin - 1) + log2L + len(planes[0]) - 2
    assert adds == sum(p is not None for ps in planes for p in ps)


def test_all_infinite_is_infinity():
    grp = Group(R)
    planes = [pm.window_planes([None] * 130, [None] * 130, grp, 16) for _ in range(3)]
    assert pm.fold_planes(planes, 16, 3, grp) == (None, 0, 0)


def test_headline_counts():
    """BN254 G1 at 2^20 (GLV half scalars: 8 windows of c = 16, 2^16 buckets, L = 8, 128 blocks): 14 planes per window - 127
    doublings, at most 112 additions"""
    rng = random.Random("planes/headline")
    grp = Group(R)
    planes = [pm.window_planes(*pairs(rng, 8192, False), grp) for _ in range(8)]
    assert all(len(p) == 14 for p in planes)
    _, dbls, adds = pm.fold_planes(planes, 16, 3, grp)
    assert dbls == 16 * 7 + 3 + 12 and adds == 112
