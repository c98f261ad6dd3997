"""Host-side mirror of the prover half of gnark-crypto's kzg package on top of the C ABI (include/gmsm.h, gmsm_poly_* /
gmsm_kzg_open*): the opening arithmetic runs on the device and the quotient is committed over resident bases.

Keeps the reference's names and meaning (ecc/bn254/kzg/kzg.go):

    claimed, H = Open(p, point, rb)                            # Open (kzg.go:180-205) over rb = G1Affine(c).register_bases(...)
    values, H = BatchOpenSinglePoint(polys, point, gamma, rb)  # BatchOpenSinglePoint (kzg.go:246-339) after the challenge
    values = PolyEval(curve, polys, point)                     # eval (kzg.go:55-63) of each polynomial
    h, value = DividePolyByXMinusA(curve, p, point)            # dividePolyByXminusA (kzg.go:565-583) and f(point)
    lagrange = ToLagrangeG1(curve, srs_g1)                     # ToLagrangeG1 (utils.go:25-64): the SRS in Lagrange form

Polynomials and field elements are numpy uint64 arrays in the layout of []fr.Element (Montgomery limbs), lowest degree
first; H is the affine commitment (G1Affine limbs). Inputs are never modified. Errors raise ValueError with the
library's text (the reference's ErrInvalidPolynomialSize wording for the size checks of Open / BatchOpenSinglePoint).
The *_device variants take raw device pointers (e.g. torch tensor.data_ptr()) and the stream that produced them.
"""
import ctypes

import numpy as np

from . import _lib
from .curves import CURVES


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _curve(curve):
    return CURVES[curve] if isinstance(curve, str) else curve


def _gid(curve):
    return _lib.GROUP_IDS[(_curve(curve).name, "g1")]


def _elem(curve, x):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(_curve(curve).fr_limbs)


def _check(rc):
    if rc:
        raise ValueError(_lib.last_error())


def _concat(curve, polys):
    nl = _curve(curve).fr_limbs
    polys = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, nl) for p in polys]
    lens = (ctypes.c_size_t * len(polys))(*[p.shape[0] for p in polys])
    flat = np.concatenate(polys) if polys else np.zeros((0, nl), dtype=np.uint64)
    return np.ascontiguousarray(flat), lens


def _host_or_none(a):
    return _ptr(a) if a.size else None


def PolyEval(curve, polys, point):
    """[eval(p, point) for p in polys] (kzg.go:55-63): a (k, fr_limbs) array."""
    c = _curve(curve)
    flat, lens = _concat(c, polys)
    out = np.zeros((len(lens), c.fr_limbs), dtype=np.uint64)
    if len(lens) == 0:
        return out
    point = _elem(c, point)
    _check(_lib.load().gmsm_poly_eval(_gid(c), _host_or_none(flat), None, lens, len(lens), _ptr(point), None, _ptr(out)))
    return out


def poly_eval_device(curve, d_polys, lens, point, stream=0):
    """PolyEval over k polynomials concatenated at device pointer d_polys (lens[i] coefficients each)."""
    c = _curve(curve)
    lens = (ctypes.c_size_t * len(lens))(*[int(x) for x in lens])
    out = np.zeros((len(lens), c.fr_limbs), dtype=np.uint64)
    point = _elem(c, point)
    _check(_lib.load().gmsm_poly_eval(_gid(c), None, d_polys, lens, len(lens), _ptr(point), stream or None, _ptr(out)))
    return out


def DividePolyByXMinusA(curve, p, point):
    """dividePolyByXminusA(p, p(point), point) (kzg.go:565-583) on a copy: returns (h, p(point)); h has len(p) - 1
    coefficients (none for len(p) == 1)."""
    c = _curve(curve)
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, c.fr_limbs)
    n = p.shape[0]
    h = np.zeros((max(n - 1, 0), c.fr_limbs), dtype=np.uint64)
    value = np.zeros(c.fr_limbs, dtype=np.uint64)
    point = _elem(c, point)
    _check(_lib.load().gmsm_poly_div_x_minus_a(_gid(c), _host_or_none(p), None, n, _ptr(point), None,
                                               _host_or_none(h), None, _ptr(value)))
    return h, value


def divide_device(curve, d_poly, n, point, d_out_h, stream=0):
    """DividePolyByXMinusA from device pointer d_poly (n coefficients) into d_out_h (n - 1); returns p(point)."""
    c = _curve(curve)
    value = np.zeros(c.fr_limbs, dtype=np.uint64)
    point = _elem(c, point)
    _check(_lib.load().gmsm_poly_div_x_minus_a(_gid(c), None, d_poly, n, _ptr(point), stream or None, None, d_out_h,
                                               _ptr(value)))
    return value


def _affine(rb, jac):
    return rb.group.jac_to_affine(jac)


def Open(p, point, rb):
    """kzg.Open(p, point, pk) with pk's G1 registered as rb (a ResidentBases of G1): returns (claimed value, H affine).
    The quotient is committed on the device without leaving it."""
    g = rb.group
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, g.fr_limbs)
    point = _elem(g.curve, point)
    claimed = np.zeros(g.fr_limbs, dtype=np.uint64)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_kzg_open(rb.handle, _host_or_none(p), None, p.shape[0], _ptr(point), None, _ptr(claimed), _ptr(jac)))
    return claimed, _affine(rb, jac)


def open_device(d_poly, n, point, rb, stream=0):
    """Open over a device polynomial of n coefficients (produced on `stream`)."""
    g = rb.group
    point = _elem(g.curve, point)
    claimed = np.zeros(g.fr_limbs, dtype=np.uint64)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_kzg_open(rb.handle, None, d_poly, n, _ptr(point), stream or None, _ptr(claimed), _ptr(jac)))
    return claimed, _affine(rb, jac)


def BatchOpenSinglePoint(polys, point, gamma, rb):
    """kzg.BatchOpenSinglePoint after the Fiat-Shamir challenge: returns (claimed values, H affine) with
    H = Commit((sum_i gamma^i f_i - sum_i gamma^i f_i(point)) / (X - point)). gamma is an argument because the transcript
    (deriveGamma over point, digests and claimed values, kzg.go:282) stays with the caller."""
    g = rb.group
    flat, lens = _concat(g.curve, polys)
    point, gamma = _elem(g.curve, point), _elem(g.curve, gamma)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_kzg_open_folded(rb.handle, _host_or_none(flat), None, lens, len(lens), _ptr(point), _ptr(gamma),
                                            None, _ptr(jac)))  # first: the size checks of the reference
    return PolyEval(g.curve, polys, point), _affine(rb, jac)


def batch_open_device(d_polys, lens, point, gamma, rb, stream=0):
    """BatchOpenSinglePoint over k polynomials concatenated at device pointer d_polys (lens[i] coefficients each)."""
    g = rb.group
    clens = (ctypes.c_size_t * len(lens))(*[int(x) for x in lens])
    point, gamma = _elem(g.curve, point), _elem(g.curve, gamma)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_kzg_open_folded(rb.handle, None, d_polys, clens, len(lens), _ptr(point), _ptr(gamma),
                                            stream or None, _ptr(jac)))
    return poly_eval_device(g.curve, d_polys, lens, point, stream), _affine(rb, jac)


ERR_POW2 = "len(coeffs) must be a power of 2"  # ToLagrangeG1, kzg/utils.go


def ToLagrangeG1(curve, points):
    """kzg.ToLagrangeG1 (utils.go:25-64) on the device: (n, 2 fp_limbs) affine G1 limbs in, the same shape out, with
    out[i] = (1/n) sum_j w^(-ij) points[j] - for an SRS [tau^j]G that is [L_i(tau)]G. n must be a power of two; inputs
    must lie in the r-torsion (as for the reference's mulGLV). Errors raise ValueError with the reference's text."""
    c = _curve(curve)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2 * c.fp_limbs)
    out = np.zeros_like(pts)
    _check(_lib.load().gmsm_to_lagrange_g1(_gid(c), _host_or_none(pts), None, pts.shape[0], None, _host_or_none(out), None))
    return out


def to_lagrange_device(curve, d_in, n, d_out, stream=0):
    """ToLagrangeG1 from device pointer d_in (n affine points, produced on `stream`) to d_out (may equal d_in)."""
    _check(_lib.load().gmsm_to_lagrange_g1(_gid(curve), None, d_in, int(n), stream or None, None, d_out))
