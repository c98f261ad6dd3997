"""Python big-int model of the ratio builders of ecc/<curve>/fr/iop/ratios.go and of fr.BatchInvert
(ecc/<curve>/fr/element.go:658-687), shared by tests/test_iop_model.py (no GPU, no library) and tests/test_gpu_iop.py.

Everything works on TRUE values mod r (plain Python ints); from_limbs / to_limbs convert the Montgomery limbs the C ABI
speaks. The loops are those of the reference, literally: the factors per index, the two serial prefix products, the batch
inversion with its zero rule, the final product. The result is Z in Lagrange basis, Regular layout (what the reference
holds before putInExpectedFormFromLagrangeRegular), n values.

A polynomial is (values, layout): n values in Lagrange basis and iop.Layout (8 Regular, 16 BitReverse)."""
import numpy as np

REGULAR, BIT_REVERSE = 8, 16


def from_limbs(curve, a):
    """(k, fr_limbs) uint64 Montgomery limbs -> list of k true values."""
    rinv = pow(curve.fr_R, -1, curve.r)
    a = np.asarray(a, dtype=np.uint64).reshape(-1, curve.fr_limbs)
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) * rinv % curve.r for row in a]


def to_limbs(curve, values):
    out = np.zeros((len(values), curve.fr_limbs), dtype=np.uint64)
    for k, v in enumerate(values):
        m = v % curve.r * curve.fr_R % curve.r
        for i in range(curve.fr_limbs):
            out[k, i] = (m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF
    return out


def generator(curve, n):
    """fr.Generator(n) (fr/generator.go:18-36) for n a power of two."""
    log2n = n.bit_length() - 1
    assert 1 << log2n == n and log2n <= curve.fr_max_order
    return pow(curve.fr_root_of_unity, 1 << (curve.fr_max_order - log2n), curve.r)


def bit_reverse_index(i, n):
    bits = n.bit_length() - 1
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def batch_invert(a, r):
    """fr.BatchInvert (element.go:658-687): the running product skips zeros, one inversion, the walk back; 0 -> 0."""
    res = [0] * len(a)
    if not a:
        return res
    zeroes = [False] * len(a)
    accumulator = 1
    for i in range(len(a)):
        if a[i] == 0:
            zeroes[i] = True
            continue
        res[i] = accumulator
        accumulator = accumulator * a[i] % r
    accumulator = pow(accumulator, -1, r)
    for i in range(len(a) - 1, -1, -1):
        if zeroes[i]:
            continue
        res[i] = res[i] * accumulator % r
        accumulator = accumulator * a[i] % r
    return res


def support(curve, nb_copies, n):
    """getSupportIdentityPermutation (ratios.go:320-361): [1, w, .., w^(n-1), g, g w, .., g^(m-1) w^(n-1)]."""
    r, w, g = curve.r, generator(curve, n), curve.fr_mult_gen
    res = [1] * (nb_copies * n)
    for i in range(1, n):
        res[i] = res[i - 1] * w % r
    for i in range(1, nb_copies):
        coset = pow(g, i, r)
        for j in range(n):
            res[i * n + j] = res[j] * coset % r
    return res


def _index(layout, i, n):
    return bit_reverse_index(i, n) if layout == BIT_REVERSE else i


def _finish(coeffs, t, r):
    n = len(coeffs)
    for i in range(2, n):
        coeffs[i] = coeffs[i] * coeffs[i - 1] % r
    for i in range(2, n):
        t[i] = t[i] * t[i - 1] % r
    t_inv = batch_invert(t[1:], r)  # the reference inverts t[1:] in chunks; 0 -> 0 in every chunk, so the cut does not show
    for i in range(1, n):
        coeffs[i] = coeffs[i] * t_inv[i - 1] % r
    return coeffs


def copy_constraint_factors(curve, entries, permutation, beta, gamma):
    """(b, d): the per-index numerator and denominator products of ratios.go:174-206, b[i], d[i] for i < n - 1."""
    r = curve.r
    n = len(entries[0][0])
    s = support(curve, len(entries), n)
    bs, ds = [], []
    for i in range(n - 1):
        b = d = 1
        for j, (values, layout) in enumerate(entries):
            p = values[_index(layout, i, n)]
            b = b * ((beta * s[i + j * n] + gamma + p) % r) % r
            d = d * ((beta * s[permutation[i + j * n]] + gamma + p) % r) % r
        bs.append(b)
        ds.append(d)
    return bs, ds


def build_ratio_copy_constraint(curve, entries, permutation, beta, gamma):
    """BuildRatioCopyConstraint (ratios.go:136-246) up to `res`: Z in Lagrange / Regular form, n true values."""
    bs, ds = copy_constraint_factors(curve, entries, permutation, beta, gamma)
    return _finish([1] + bs, [1] + ds, curve.r)


def shuffled_factors(curve, numerator, denominator, beta):
    r = curve.r
    n = len(numerator[0][0])
    bs, ds = [], []
    for i in range(n - 1):
        b = d = 1
        for (pv, pl), (qv, ql) in zip(numerator, denominator):
            b = b * ((beta - pv[_index(pl, i, n)]) % r) % r
            d = d * ((beta - qv[_index(ql, i, n)]) % r) % r
        bs.append(b)
        ds.append(d)
    return bs, ds


def build_ratio_shuffled_vectors(curve, numerator, denominator, beta):
    """BuildRatioShuffledVectors (ratios.go:45-127) up to `res`: Z in Lagrange / Regular form, n true values."""
    bs, ds = shuffled_factors(curve, numerator, denominator, beta)
    return _finish([1] + bs, [1] + ds, curve.r)
