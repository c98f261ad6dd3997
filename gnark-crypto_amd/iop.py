"""Host-side mirror of the ratio builders of gnark-crypto's fr/iop package, and of fr.BatchInvert, on top of the C ABI
(include/gmsm.h: gmsm_iop_ratio_copy_constraint, gmsm_iop_ratio_shuffled, gmsm_fr_batch_invert).

Keeps the reference's names and meaning (ecc/bn254/fr/iop/ratios.go, polynomial.go; ecc/bn254/fr/element.go):

    form = Form(Lagrange, Regular)
    Z = BuildRatioCopyConstraint("bn254", entries, permutation, beta, gamma, form)       # ratios.go:136-246
    Z = BuildRatioShuffledVectors("bn254", numerator, denominator, beta, form)            # ratios.go:45-127
    inv = BatchInvert("bn254", a)                                                         # element.go:658-687, 0 -> 0

A polynomial is a triple (coeffs, basis, layout): coeffs a numpy uint64 array (n, fr_limbs) in the layout of []fr.Element
(Montgomery limbs), basis one of Canonical / Lagrange / LagrangeCoset, layout Regular / BitReverse (the reference's
values). The C entries take Lagrange basis only; the reference's ToLagrange on the inputs (polynomial.go:296-315) is done
here through fft.Domain, on copies: inputs are never modified. Errors raise ValueError with the reference's text
(ErrNumberPolynomials, ErrInconsistentSize, ErrSizeNotPowerOfTwo, ErrInconsistentSizeDomain) or the library's.
The *_device variants take raw device pointers (e.g. torch tensor.data_ptr()) of Lagrange-basis vectors and the stream
that produced them.

The rest of the package (polynomial.go, quotient.go) over gmsm_iop_to_basis, gmsm_iop_evaluate and
gmsm_iop_divide_by_x_minus_one:

    p = NewPolynomial("bn254", coeffs, Form(Canonical, Regular))      # polynomial.go:73-78, coeffs shared, not copied
    p.ToLagrange(d); p.ToCanonical(d); p.ToLagrangeCoset(d)           # :287-390, grow included; in place, return p
    p.ToRegular(); p.ToBitReverse(); p.Shift(1); p.GetCoeff(i); p.Clone(); p.ShallowClone(); p.Size(); p.SetSize(n)
    y = p.Evaluate(x)                                                 # :104-132; 0 for x in the domain of a Lagrange basis
    q = DivideByXMinusOne(h, (small, big))                            # quotient.go:21-53: Canonical / Regular

with to_basis_device, evaluate_device and divide_by_x_minus_one_device over raw device pointers. iop.Evaluate(f Expression,
...) takes an arbitrary function and stays on the host.
"""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from . import fft
from .curves import CURVES

# iop.Basis, iop.Layout (polynomial.go:20-34)
Canonical, Lagrange, LagrangeCoset = 1, 2, 4
Regular, BitReverse = 8, 16
Form = namedtuple("Form", ["Basis", "Layout"])


class Basis:
    Canonical, Lagrange, LagrangeCoset = Canonical, Lagrange, LagrangeCoset


class Layout:
    Regular, BitReverse = Regular, BitReverse


ErrInconsistentSize = "the sizes of the polynomial must be the same as the size of the domain"
ErrNumberPolynomials = "the number of polynomials in the denominator and the numerator must be the same"
ErrSizeNotPowerOfTwo = "the size of the polynomials must be a power of two"
ErrInconsistentSizeDomain = "the size of the domain must be consistent with the size of the polynomials"

_u32p = ctypes.POINTER(ctypes.c_uint32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _curve(curve):
    return CURVES[curve] if isinstance(curve, str) else curve


def _gid(curve):
    return _lib.GROUP_IDS[(_curve(curve).name, "g1")]


def _elem(c, x):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(c.fr_limbs)


def _check(rc):
    if rc:
        raise ValueError(_lib.last_error())


def _layouts(values):
    return np.ascontiguousarray([int(v) for v in values], dtype=np.uint32)


def BatchInvert(curve, a):
    """fr.BatchInvert(a) (element.go:658-687): a new array with 1 / a[i], and 0 where a[i] is 0."""
    c = _curve(curve)
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, c.fr_limbs)
    out = np.zeros_like(a)
    if a.shape[0]:
        _check(_lib.load().gmsm_fr_batch_invert(_gid(c), _ptr(a), None, a.shape[0], None, _ptr(out), None))
    return out


def batch_invert_device(curve, d_a, n, d_out, stream=0):
    """BatchInvert from device pointer d_a (n elements, produced on `stream`) to d_out (may equal d_a)."""
    _check(_lib.load().gmsm_fr_batch_invert(_gid(curve), None, d_a, int(n), stream or None, None, d_out))


def _polys(c, entries):
    out = []
    for coeffs, basis, layout in entries:
        out.append((np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, c.fr_limbs), int(basis), int(layout)))
    return out


def _check_size(*lists):
    # checkSize (ratios.go:277-291): every polynomial has the length of the first
    n = lists[0][0][0].shape[0]
    for pols in lists:
        for p in pols:
            if p[0].shape[0] != n:
                raise ValueError(ErrInconsistentSize)
    return n


def _build_domain(c, n, domain):
    # buildDomain (ratios.go:295-313); returns the domain and whether it was made here
    if n == 0 or n & (n - 1):
        raise ValueError(ErrSizeNotPowerOfTwo)
    if domain is None:
        return fft.NewDomain(c, n), True
    if domain.Cardinality != n:
        raise ValueError(ErrInconsistentSizeDomain)
    return domain, False


def _to_lagrange(d, p):
    """(*Polynomial).ToLagrange (polynomial.go:287-318) on a copy: (coeffs, layout) in Lagrange basis."""
    coeffs, basis, layout = p
    if basis == Lagrange and layout in (Regular, BitReverse):
        return coeffs, layout
    form = (basis, layout)
    if form == (Canonical, Regular):
        return d.FFT(coeffs, fft.DIF), BitReverse
    if form == (Canonical, BitReverse):
        return d.FFT(coeffs, fft.DIT), Regular
    if form == (LagrangeCoset, Regular):
        return d.FFT(d.FFTInverse(coeffs, fft.DIF, fft.OnCoset()), fft.DIT), Regular
    if form == (LagrangeCoset, BitReverse):
        return d.FFT(d.FFTInverse(coeffs, fft.DIT, fft.OnCoset()), fft.DIF), BitReverse
    raise ValueError("unknown ID")  # the reference panics


def _lagrange_inputs(d, pols):
    conv = [_to_lagrange(d, p) for p in pols]
    return np.ascontiguousarray(np.concatenate([x[0] for x in conv])), _layouts(x[1] for x in conv)


def BuildRatioCopyConstraint(curve, entries, permutation, beta, gamma, expectedForm, domain=None):
    """iop.BuildRatioCopyConstraint (ratios.go:136-246): the (n, fr_limbs) coefficients of Z in expectedForm."""
    c = _curve(curve)
    pols = _polys(c, entries)
    if not pols:
        raise ValueError("gmsm_iop_ratio_copy_constraint: no polynomial (m == 0)")  # the reference indexes entries[0]
    n = _check_size(pols)
    d, own = _build_domain(c, n, domain)
    try:
        flat, layouts = _lagrange_inputs(d, pols)
        perm = np.ascontiguousarray(permutation, dtype=np.int64).reshape(-1)
        if perm.shape[0] < len(pols) * n:
            raise ValueError("gmsm_iop_ratio_copy_constraint: the permutation has fewer than m * n entries")
        beta, gamma = _elem(c, beta), _elem(c, gamma)
        out = np.zeros((n, c.fr_limbs), dtype=np.uint64)
        _check(_lib.load().gmsm_iop_ratio_copy_constraint(d.handle, _ptr(flat), None, len(pols), layouts.ctypes.data_as(_u32p), _ptr(perm), None,
                                                          _ptr(beta), _ptr(gamma), int(expectedForm[0]), int(expectedForm[1]), None,
                                                          _ptr(out), None))
        return out
    finally:
        if own:
            d.release()


def BuildRatioShuffledVectors(curve, numerator, denominator, beta, expectedForm, domain=None):
    """iop.BuildRatioShuffledVectors (ratios.go:45-127): the (n, fr_limbs) coefficients of Z in expectedForm."""
    c = _curve(curve)
    if len(numerator) != len(denominator):
        raise ValueError(ErrNumberPolynomials)
    num, den = _polys(c, numerator), _polys(c, denominator)
    if not num:
        raise ValueError("gmsm_iop_ratio_shuffled: no polynomial (m == 0)")  # the reference indexes numerator[0]
    n = _check_size(num, den)
    d, own = _build_domain(c, n, domain)
    try:
        fnum, lnum = _lagrange_inputs(d, num)
        fden, lden = _lagrange_inputs(d, den)
        beta = _elem(c, beta)
        out = np.zeros((n, c.fr_limbs), dtype=np.uint64)
        _check(_lib.load().gmsm_iop_ratio_shuffled(d.handle, _ptr(fnum), None, _ptr(fden), None, len(num), lnum.ctypes.data_as(_u32p),
                                                   lden.ctypes.data_as(_u32p), _ptr(beta), int(expectedForm[0]), int(expectedForm[1]), None,
                                                   _ptr(out), None))
        return out
    finally:
        if own:
            d.release()


def build_ratio_copy_constraint_device(domain, d_entries, layouts, d_perm, beta, gamma, expectedForm, d_out, stream=0):
    """BuildRatioCopyConstraint over m = len(layouts) Lagrange-basis polynomials concatenated at device pointer d_entries
    (domain.Cardinality elements each) and the int64 permutation at d_perm, both produced on `stream`; Z goes to d_out."""
    c = domain.curve
    lay = _layouts(layouts)
    beta, gamma = _elem(c, beta), _elem(c, gamma)
    _check(_lib.load().gmsm_iop_ratio_copy_constraint(domain.handle, None, d_entries, len(lay), lay.ctypes.data_as(_u32p), None, d_perm,
                                                      _ptr(beta), _ptr(gamma), int(expectedForm[0]), int(expectedForm[1]), stream or None,
                                                      None, d_out))


def build_ratio_shuffled_vectors_device(domain, d_num, num_layouts, d_den, den_layouts, beta, expectedForm, d_out, stream=0):
    """BuildRatioShuffledVectors over Lagrange-basis polynomials concatenated at device pointers d_num / d_den."""
    c = domain.curve
    if len(num_layouts) != len(den_layouts):
        raise ValueError(ErrNumberPolynomials)
    ln, ld = _layouts(num_layouts), _layouts(den_layouts)
    beta = _elem(c, beta)
    _check(_lib.load().gmsm_iop_ratio_shuffled(domain.handle, None, d_num, None, d_den, len(ln), ln.ctypes.data_as(_u32p),
                                               ld.ctypes.data_as(_u32p), _ptr(beta), int(expectedForm[0]), int(expectedForm[1]),
                                               stream or None, None, d_out))


# ---- iop.Polynomial (polynomial.go) and iop.DivideByXMinusOne (quotient.go) over gmsm_iop_to_basis, gmsm_iop_evaluate and
# gmsm_iop_divide_by_x_minus_one
ErrMustBeLagrangeCoset = "the basis must be LagrangeCoset"


def to_basis_device(domain, d_a, length, form, to_basis, stream=0):
    """ToLagrange / ToCanonical / ToLagrangeCoset in place on the domain.Cardinality elements at device pointer d_a, of which
    the first `length` are given (the rest is zeroed: the reference's grow); returns the layout the reference leaves."""
    out_layout = ctypes.c_int(0)
    _check(_lib.load().gmsm_iop_to_basis(domain.handle, None, d_a, int(length), int(form[0]), int(form[1]), int(to_basis), stream or None,
                                         ctypes.byref(out_layout)))
    return out_layout.value


def evaluate_device(curve, d_polys, k, length, size, basis, layouts, shift, coset, x, stream=0):
    """Evaluate of k polynomials of `length` coefficients concatenated at device pointer d_polys: (k, fr_limbs) values."""
    c = _curve(curve)
    lay = _layouts(layouts)
    out = np.zeros((int(k), c.fr_limbs), dtype=np.uint64)
    cs = None if coset is None else _elem(c, coset)
    _check(_lib.load().gmsm_iop_evaluate(_gid(c), None, d_polys, int(k), int(length), int(size), int(basis), lay.ctypes.data_as(_u32p), int(shift),
                                         None if cs is None else _ptr(cs), _ptr(_elem(c, x)), stream or None, _ptr(out)))
    return out


def divide_by_x_minus_one_device(domains, d_a, form, shift, d_out, stream=0):
    """DivideByXMinusOne of the domains[1].Cardinality elements at device pointer d_a (a polynomial of size
    domains[0].Cardinality, shifted by `shift`) into d_out: Canonical basis, Regular layout."""
    _check(_lib.load().gmsm_iop_divide_by_x_minus_one(domains[0].handle, domains[1].handle, None, d_a, int(form[0]), int(form[1]), int(shift),
                                                      stream or None, None, d_out))


class Polynomial:
    """iop.Polynomial (polynomial.go:62-78): coefficients (a numpy (n, fr_limbs) array, shared, not copied), Basis, Layout, shift,
    size and coset. It iterates as (coeffs, basis, layout), so the BuildRatio* functions above take it as it is."""

    def __init__(self, curve, coeffs, form):
        self.curve = _curve(curve)
        a = np.ascontiguousarray(coeffs, dtype=np.uint64)  # the array itself when it is already contiguous uint64: shared
        self.coefficients = a if a.ndim == 2 and a.shape[1] == self.curve.fr_limbs else a.reshape(-1, self.curve.fr_limbs)
        self.Basis, self.Layout = int(form[0]), int(form[1])
        self.shift, self.size = 0, self.coefficients.shape[0]
        self.coset = np.zeros(self.curve.fr_limbs, dtype=np.uint64)

    def __iter__(self):
        return iter((self.coefficients, self.Basis, self.Layout))

    @property
    def Form(self):
        return Form(self.Basis, self.Layout)

    def Shift(self, shift):
        self.shift = int(shift)
        return self

    def Size(self):
        return self.size

    def SetSize(self, size):
        self.size = int(size)

    def ShallowClone(self):
        res = Polynomial(self.curve, self.coefficients, (self.Basis, self.Layout))
        res.coefficients = self.coefficients  # the same vector
        res.shift, res.size, res.coset = self.shift, self.size, self.coset.copy()
        return res

    def Clone(self):
        res = self.ShallowClone()
        res.coefficients = self.coefficients.copy()
        return res

    def Coefficients(self):
        return self.coefficients

    def GetCoeff(self, i):
        """polynomial.go:151-163: the i-th entry, taking shift and layout in account"""
        n = self.coefficients.shape[0]
        j = (i + (n // self.size) * self.shift) % n
        if self.Layout != Regular:
            bits = n.bit_length() - 1
            j = int(format(j, "0%db" % bits)[::-1], 2) if bits else 0
        return self.coefficients[j]

    def _to_layout(self, layout):
        if self.Layout != layout:
            self.coefficients[:] = fft.BitReverse(self.curve, self.coefficients)
            self.Layout = layout
        return self

    def ToRegular(self):
        return self._to_layout(Regular)

    def ToBitReverse(self):
        return self._to_layout(BitReverse)

    def _to_basis(self, d, basis):
        n, card = self.coefficients.shape[0], d.Cardinality
        buf = self.coefficients
        if n < card:  # grow: the entry zeroes the tail
            buf = np.empty((card, self.curve.fr_limbs), dtype=np.uint64)
            buf[:n] = self.coefficients
        out_layout = ctypes.c_int(0)
        _check(_lib.load().gmsm_iop_to_basis(d.handle, _ptr(buf), None, n, self.Basis, self.Layout, basis, None, ctypes.byref(out_layout)))
        self.coefficients, self.Basis, self.Layout = buf, basis, out_layout.value
        return self

    def ToLagrange(self, d):
        return self._to_basis(d, Lagrange)

    def ToCanonical(self, d):
        return self._to_basis(d, Canonical)

    def ToLagrangeCoset(self, d):
        self.coset = np.array(d.FrMultiplicativeGen, dtype=np.uint64)  # cosetTable[1], whatever the form (polynomial.go:364)
        return self._to_basis(d, LagrangeCoset)

    def Evaluate(self, x):
        """(*Polynomial).Evaluate (polynomial.go:104-132): one fr.Element. A shift outside 0..5 raises ValueError."""
        if self.shift < 0:
            raise ValueError("gmsm_iop_evaluate: shift %d is outside 0..5 (the reference evaluates at 0 there)" % self.shift)
        lay = _layouts([self.Layout])
        out = np.zeros(self.curve.fr_limbs, dtype=np.uint64)
        _check(_lib.load().gmsm_iop_evaluate(_gid(self.curve), _ptr(self.coefficients), None, 1, self.coefficients.shape[0], self.size, self.Basis,
                                             lay.ctypes.data_as(_u32p), self.shift, _ptr(self.coset), _ptr(_elem(self.curve, x)), None, _ptr(out)))
        return out


def NewPolynomial(curve, coeffs, form):
    """iop.NewPolynomial (polynomial.go:73-78): the coefficients are not copied."""
    return Polynomial(curve, coeffs, form)


def DivideByXMinusOne(a, domains):
    """iop.DivideByXMinusOne (quotient.go:21-53): a (LagrangeCoset, len = domains[1].Cardinality, size = domains[0].Cardinality)
    divided by X^size - 1: a new Polynomial, Canonical / Regular, size = a.size. a is not modified."""
    if a.Basis != LagrangeCoset:
        raise ValueError(ErrMustBeLagrangeCoset)
    out = np.zeros_like(a.coefficients)
    _check(_lib.load().gmsm_iop_divide_by_x_minus_one(domains[0].handle, domains[1].handle, _ptr(a.coefficients), None, a.Basis, a.Layout,
                                                      a.shift % (1 << 64), None, _ptr(out), None))
    res = Polynomial(a.curve, out, (Canonical, Regular))
    res.size = a.size
    return res
