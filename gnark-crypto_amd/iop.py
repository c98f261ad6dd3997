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
