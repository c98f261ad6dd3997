"""Python big-int model of iop.Polynomial and iop.DivideByXMinusOne (ecc/<curve>/fr/iop/polynomial.go, quotient.go), shared
by tests/test_iop_poly_model.py (no GPU, no library) and tests/test_gpu_iop_poly.py.

Everything works on TRUE values mod r (plain Python ints; iop_model.from_limbs / to_limbs convert the Montgomery limbs the C
ABI speaks). Four parts:
  - the reference's evaluation loops, literally: Evaluate's coset and shift rules, Horner in either layout, and the
    evalLagrange loop with its running `li` and the batch inversion's zero rule
  - the conversion switch of ToLagrange / ToCanonical / ToLagrangeCoset (with grow) over a plain radix-2 NTT
  - GetCoeff
  - DivideByXMinusOne with evaluateXnMinusOneDomainBigCoset"""
import iop_model as M

CANONICAL, LAGRANGE, LAGRANGE_COSET = 1, 2, 4
REGULAR, BIT_REVERSE = M.REGULAR, M.BIT_REVERSE
DIT, DIF = 0, 1


def next_power_of_two(n):
    return 1 << max(n - 1, 0).bit_length()


class Domain:
    """fft.Domain (fr/fft/domain.go:24-110) with the default coset shift: the constants only."""

    def __init__(self, curve, m):
        self.curve = curve
        self.cardinality = next_power_of_two(m)
        self.generator = M.generator(curve, self.cardinality)
        self.fr_multiplicative_gen = curve.fr_mult_gen


class Polynomial:
    """iop.Polynomial (polynomial.go:62-78): a list of true values, the form, shift, size and coset."""

    def __init__(self, coeffs, basis, layout):
        self.coefficients = list(coeffs)
        self.basis, self.layout = basis, layout
        self.shift, self.size, self.coset = 0, len(self.coefficients), 0

    def clone(self):
        p = Polynomial(self.coefficients, self.basis, self.layout)
        p.shift, p.size, p.coset = self.shift, self.size, self.coset
        return p


# ---- a plain radix-2 NTT and the reference's transforms on top of it
def ntt(values, w, r):
    """[sum_j values[j] w^(j k) for k], natural order in and out; len(values) a power of two"""
    n = len(values)
    if n == 1:
        return list(values)
    even, odd = ntt(values[0::2], w * w % r, r), ntt(values[1::2], w * w % r, r)
    out, t = [0] * n, 1
    for k in range(n // 2):
        o = t * odd[k] % r
        out[k], out[k + n // 2] = (even[k] + o) % r, (even[k] - o) % r
        t = t * w % r
    return out


def _reorder(a):
    n = len(a)
    return [a[M.bit_reverse_index(i, n)] for i in range(n)]


def fft(d, a, decimation, coset=False):
    """(*Domain).FFT (fft.go:31-82): DIF natural in, bit-reversed out; DIT the reverse; OnCoset scales coefficient j by g^j first"""
    r = d.curve.r
    nat = list(a) if decimation == DIF else _reorder(a)
    if coset:
        nat = [v * pow(d.fr_multiplicative_gen, j, r) % r for j, v in enumerate(nat)]
    out = ntt(nat, d.generator, r)
    return _reorder(out) if decimation == DIF else out


def fft_inverse(d, a, decimation, coset=False):
    """(*Domain).FFTInverse (fft.go:88-196): the inverse transform, 1/n, and on the coset coefficient j times g^-j"""
    r = d.curve.r
    nat = list(a) if decimation == DIF else _reorder(a)
    ninv = pow(d.cardinality, -1, r)
    out = [v * ninv % r for v in ntt(nat, pow(d.generator, -1, r), r)]
    if coset:
        ginv = pow(d.fr_multiplicative_gen, -1, r)
        out = [v * pow(ginv, j, r) % r for j, v in enumerate(out)]
    return _reorder(out) if decimation == DIF else out


# ---- the conversion switch (polynomial.go:287-390), case by case
def _grow(p, new_size):
    if new_size > len(p.coefficients):
        p.coefficients += [0] * (new_size - len(p.coefficients))


def to_lagrange(p, d):
    form = (p.basis, p.layout)
    _grow(p, d.cardinality)
    if form == (CANONICAL, REGULAR):
        p.layout = BIT_REVERSE
        p.coefficients = fft(d, p.coefficients, DIF)
    elif form == (CANONICAL, BIT_REVERSE):
        p.layout = REGULAR
        p.coefficients = fft(d, p.coefficients, DIT)
    elif form[0] == LAGRANGE:
        return p
    elif form == (LAGRANGE_COSET, REGULAR):
        p.layout = REGULAR
        p.coefficients = fft(d, fft_inverse(d, p.coefficients, DIF, coset=True), DIT)
    elif form == (LAGRANGE_COSET, BIT_REVERSE):
        p.layout = BIT_REVERSE
        p.coefficients = fft(d, fft_inverse(d, p.coefficients, DIT, coset=True), DIF)
    else:
        raise ValueError("unknown ID")
    p.basis = LAGRANGE
    return p


def to_canonical(p, d):
    form = (p.basis, p.layout)
    _grow(p, d.cardinality)
    if form[0] == CANONICAL:
        return p
    if form == (LAGRANGE, REGULAR):
        p.layout = BIT_REVERSE
        p.coefficients = fft_inverse(d, p.coefficients, DIF)
    elif form == (LAGRANGE, BIT_REVERSE):
        p.layout = REGULAR
        p.coefficients = fft_inverse(d, p.coefficients, DIT)
    elif form == (LAGRANGE_COSET, REGULAR):
        p.layout = BIT_REVERSE
        p.coefficients = fft_inverse(d, p.coefficients, DIF, coset=True)
    elif form == (LAGRANGE_COSET, BIT_REVERSE):
        p.layout = REGULAR
        p.coefficients = fft_inverse(d, p.coefficients, DIT, coset=True)
    else:
        raise ValueError("unknown ID")
    p.basis = CANONICAL
    return p


def to_lagrange_coset(p, d):
    p.coset = d.fr_multiplicative_gen  # cosetTable[1], set whatever the form
    form = (p.basis, p.layout)
    _grow(p, d.cardinality)
    if form == (CANONICAL, REGULAR):
        p.layout = BIT_REVERSE
        p.coefficients = fft(d, p.coefficients, DIF, coset=True)
    elif form == (CANONICAL, BIT_REVERSE):
        p.layout = REGULAR
        p.coefficients = fft(d, p.coefficients, DIT, coset=True)
    elif form == (LAGRANGE, REGULAR):
        p.layout = REGULAR
        p.coefficients = fft(d, fft_inverse(d, p.coefficients, DIF), DIT, coset=True)
    elif form == (LAGRANGE, BIT_REVERSE):
        p.layout = BIT_REVERSE
        p.coefficients = fft(d, fft_inverse(d, p.coefficients, DIT), DIF, coset=True)
    elif form[0] == LAGRANGE_COSET:
        return p
    else:
        raise ValueError("unknown ID")
    p.basis = LAGRANGE_COSET
    return p


TO = {LAGRANGE: to_lagrange, CANONICAL: to_canonical, LAGRANGE_COSET: to_lagrange_coset}


def to_regular(p):
    if p.layout != REGULAR:
        p.coefficients, p.layout = _reorder(p.coefficients), REGULAR
    return p


def to_bit_reverse(p):
    if p.layout != BIT_REVERSE:
        p.coefficients, p.layout = _reorder(p.coefficients), BIT_REVERSE
    return p


# ---- Evaluate (polynomial.go:104-132) and evaluate (:198-261)
def _evaluate(curve, coefficients, basis, layout, x):
    r = curve.r
    size_p = len(coefficients)
    res = 0
    if basis == CANONICAL:
        for i in range(size_p - 1, -1, -1):
            idx = i if layout == REGULAR else M.bit_reverse_index(i, size_p)
            res = (res * x + coefficients[idx]) % r
        return res
    # evalLagrange
    w = M.generator(curve, next_power_of_two(size_p))
    accw, dens = 1, []
    for _ in range(size_p):
        dens.append((x - accw) % r)
        accw = accw * w % r
    invdens = M.batch_invert(dens, r)
    li = pow(size_p, -1, r) * ((pow(x, size_p, r) - 1) % r) % r  # 1/n * (x^n - 1)
    for i in range(size_p):
        idx = i if layout == REGULAR else M.bit_reverse_index(i, size_p)
        li = li * invdens[i] % r
        res = (res + li * coefficients[idx]) % r
        li = li * dens[i] % r * w % r
    return res


def evaluate(curve, p, x):
    """(*Polynomial).Evaluate for shift in 0..5 (beyond, the reference multiplies by an element it never set: not modelled)"""
    r = curve.r
    if p.basis == LAGRANGE_COSET:
        x = x * (pow(p.coset, -1, r) if p.coset else 0) % r  # fr.Div: 0^-1 = 0
    if p.shift == 0:
        return _evaluate(curve, p.coefficients, p.basis, p.layout, x)
    assert 0 < p.shift <= 5
    gen = M.generator(curve, next_power_of_two(p.size))
    x = x * pow(gen, p.shift, r) % r
    return _evaluate(curve, p.coefficients, p.basis, p.layout, x)


# ---- GetCoeff (polynomial.go:151-163)
def get_coeff(p, i):
    n = len(p.coefficients)
    rho = n // p.size
    j = (i + rho * p.shift) % n
    return p.coefficients[j if p.layout == REGULAR else M.bit_reverse_index(j, n)]


# ---- DivideByXMinusOne (quotient.go:21-79)
def evaluate_xn_minus_one_domain_big_coset(domains):
    small, big = domains
    r = big.curve.r
    ratio = big.cardinality // small.cardinality
    res = [0] * ratio
    res[0] = pow(big.fr_multiplicative_gen, small.cardinality, r)
    t = pow(big.generator, small.cardinality, r)
    for i in range(1, ratio):
        res[i] = res[i - 1] * t % r
        res[i - 1] = (res[i - 1] - 1) % r
    res[-1] = (res[-1] - 1) % r
    return M.batch_invert(res, r)


def divide_by_x_minus_one(a, domains):
    if a.basis != LAGRANGE_COSET:
        raise ValueError("the basis must be LagrangeCoset")
    r = domains[1].curve.r
    inv = evaluate_xn_minus_one_domain_big_coset(domains)
    n = len(a.coefficients)
    rho = n // a.size
    res = Polynomial([0] * n, LAGRANGE_COSET, BIT_REVERSE)
    res.size = a.size
    for i in range(n):
        res.coefficients[M.bit_reverse_index(i, n)] = get_coeff(a, i) * inv[i % rho] % r
    return to_canonical(res, domains[1])
