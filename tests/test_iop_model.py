"""tests/iop_model.py pinned with the reference's own test identities (no GPU, no library): for inputs invariant under the
permutation the accumulating ratio closes - Z[n-1] b_(n-1) / d_(n-1) = 1 (ratios_test.go:60-102 for the shuffled vectors,
:205-252 for the copy constraint) -, for other inputs it does not; the layout flag only re-indexes; BatchInvert keeps the
reference's zero rule; the limb conversion round-trips."""
import importlib
import random

import pytest

import iop_model as M

curves = importlib.import_module("gnark-crypto_amd.curves")  # tests/conftest.py puts the repository root on sys.path
CURVES = ["bn254", "bls12_381", "bw6_761"]
N, NB = 8, 4  # sizePolynomials, nbPolynomials of the reference's tests


def rnd_for(*tags):
    return random.Random("iop-model-" + "-".join(str(t) for t in tags))


def invariant_entries(rnd, r, n, m):
    """getInvariantEntriesUnderPermutation (ratios_test.go:186-203): sigma = (0 1)(2 3)..., equal values on each pair."""
    entries = []
    for _ in range(m):
        v = [0] * n
        for j in range(n // 2):
            v[2 * j] = v[2 * j + 1] = rnd.randrange(r)
        entries.append((v, M.REGULAR))
    perm = [0] * (m * n)
    for i in range(m * n // 2):
        perm[2 * i], perm[2 * i + 1] = 2 * i + 1, 2 * i
    return entries, perm


def permuted_polynomials(rnd, r, n, m):
    """getPermutedPolynomials (ratios_test.go:20-58): the denominators are the numerators, concatenated and permuted."""
    num = [[rnd.randrange(r) for _ in range(n)] for _ in range(m)]
    sigma, a = [], 3
    for _ in range(n * m):
        sigma.append(a)
        a = (a + 3) % (n * m)
    den = [[0] * n for _ in range(m)]
    for i, s in enumerate(sigma):
        den[i // n][i % n] = num[s // n][s % n]
    return [(v, M.REGULAR) for v in num], [(v, M.REGULAR) for v in den]


def bit_reversed(values):
    n = len(values)
    return [values[M.bit_reverse_index(i, n)] for i in range(n)]


@pytest.mark.parametrize("curve", CURVES)
def test_copy_constraint_ratio_closes_on_invariant_entries(curve):
    c = curves.CURVES[curve]
    r, rnd = c.r, rnd_for(curve, "cc")
    entries, sigma = invariant_entries(rnd, r, N, NB)
    beta, gamma = rnd.randrange(r), rnd.randrange(r)
    z = M.build_ratio_copy_constraint(c, entries, sigma, beta, gamma)
    assert len(z) == N and z[0] == 1
    supp = M.support(c, NB, N)
    b = d = 1
    for i in range(NB):
        b = b * (beta * supp[(i + 1) * N - 1] + entries[i][0][N - 1] + gamma) % r
        d = d * (beta * supp[sigma[(i + 1) * N - 1]] + entries[i][0][N - 1] + gamma) % r
    assert b * z[N - 1] * pow(d, -1, r) % r == 1
    # the same entries given bit-reversed (ratios_test.go:255-270)
    rev = [(bit_reversed(v), M.BIT_REVERSE) for v, _ in entries]
    assert M.build_ratio_copy_constraint(c, rev, sigma, beta, gamma) == z
    # entries that are not invariant: the ratio does not close
    bad = [(list(v), l) for v, l in entries]
    bad[1][0][3] = (bad[1][0][3] + 1) % r
    zb = M.build_ratio_copy_constraint(c, bad, sigma, beta, gamma)
    b = d = 1
    for i in range(NB):
        b = b * (beta * supp[(i + 1) * N - 1] + bad[i][0][N - 1] + gamma) % r
        d = d * (beta * supp[sigma[(i + 1) * N - 1]] + bad[i][0][N - 1] + gamma) % r
    assert b * zb[N - 1] * pow(d, -1, r) % r != 1


@pytest.mark.parametrize("curve", CURVES)
def test_shuffled_ratio_closes_on_permuted_vectors(curve):
    c = curves.CURVES[curve]
    r, rnd = c.r, rnd_for(curve, "sv")
    num, den = permuted_polynomials(rnd, r, N, NB)
    beta = rnd.randrange(r)
    z = M.build_ratio_shuffled_vectors(c, num, den, beta)
    assert len(z) == N and z[0] == 1

    def closes(num, den, z):
        b = d = 1
        for i in range(NB):
            b = b * (beta - num[i][0][N - 1]) % r
            d = d * (beta - den[i][0][N - 1]) % r
        return b * z[N - 1] * pow(d, -1, r) % r == 1
    assert closes(num, den, z)
    rnum = [(bit_reversed(v), M.BIT_REVERSE) for v, _ in num]
    rden = [(bit_reversed(v), M.BIT_REVERSE) for v, _ in den]
    assert M.build_ratio_shuffled_vectors(c, rnum, rden, beta) == z
    assert M.build_ratio_shuffled_vectors(c, rnum, den, beta) == z  # the flag is per polynomial
    bad = [(list(v), l) for v, l in den]
    bad[2][0][5] = (bad[2][0][5] + 1) % r
    assert not closes(num, bad, M.build_ratio_shuffled_vectors(c, num, bad, beta))


@pytest.mark.parametrize("curve", CURVES)
def test_identity_permutation_gives_ones_and_a_zero_denominator_zeroes_the_tail(curve):
    c = curves.CURVES[curve]
    r, rnd = c.r, rnd_for(curve, "id")
    n, m = 8, 3
    entries = [([rnd.randrange(r) for _ in range(n)], M.REGULAR) for _ in range(m)]
    beta, gamma = rnd.randrange(r), rnd.randrange(r)
    ident = list(range(m * n))
    assert M.build_ratio_copy_constraint(c, entries, ident, beta, gamma) == [1] * n
    perm = list(ident)
    rnd.shuffle(perm)
    z = M.build_ratio_copy_constraint(c, entries, perm, beta, gamma)
    k, j = 3, 1
    supp = M.support(c, m, n)
    entries[j][0][k] = (-beta * supp[perm[k + j * n]] - gamma) % r  # d_k = 0
    z0 = M.build_ratio_copy_constraint(c, entries, perm, beta, gamma)
    assert z0[:k + 1] == z[:k + 1] and z0[k + 1:] == [0] * (n - k - 1)


def test_support_and_generator():
    c = curves.CURVES["bn254"]
    n, m = 8, 3
    w = M.generator(c, n)
    assert pow(w, n, c.r) == 1 and pow(w, n // 2, c.r) == c.r - 1
    s = M.support(c, m, n)
    assert all(s[p] == pow(c.fr_mult_gen, p // n, c.r) * pow(w, p % n, c.r) % c.r for p in range(m * n))
    assert M.generator(c, 1) == 1 and M.support(c, 2, 1) == [1, c.fr_mult_gen]


@pytest.mark.parametrize("curve", CURVES)
def test_batch_invert_zero_rule_and_limbs(curve):
    c = curves.CURVES[curve]
    r, rnd = c.r, rnd_for(curve, "inv")
    a = [rnd.randrange(1, r) for _ in range(9)]
    a[0] = a[4] = a[8] = 0
    inv = M.batch_invert(a, r)
    assert [x * y % r for x, y in zip(a, inv)] == [0, 1, 1, 1, 0, 1, 1, 1, 0]
    assert inv[0] == inv[4] == inv[8] == 0
    assert M.batch_invert([0, 0], r) == [0, 0] and M.batch_invert([], r) == []
    assert M.from_limbs(c, M.to_limbs(c, a)) == a
    assert M.to_limbs(c, [1])[0].tolist() == [(c.fr_R % r >> (64 * i)) & (2**64 - 1) for i in range(c.fr_limbs)]
    assert [M.bit_reverse_index(i, 8) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and M.bit_reverse_index(0, 1) == 0
