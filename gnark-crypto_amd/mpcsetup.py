"""Host-side mirror of the point updates of gnark-crypto's SRS ceremony (ecc/<curve>/mpcsetup, ecc/<curve>/kzg/mpcsetup.go)
on top of the C ABI (include/gmsm.h: gmsm_batch_scale, gmsm_update_monomials, gmsm_linear_combinations). Every point is
multiplied by its own scalar on the device, one lane per point (csrc/gmsm_scale.h).

    A = UpdateMonomialsG1(curve, A, r)                 # A[i] <- r^i A[i]  (mpcsetup.UpdateMonomialsG1, what Contribute and Seal call)
    A = UpdateMonomialsG2(curve, A, r)                 # the same over G2 points
    A = ScaleG1(curve, A, s) / ScaleG2                 # A[i] <- s A[i]    (the slice cases of mpcsetup.UpdateValues)
    A = BatchScaleG1(curve, A, scalars) / BatchScaleG2 # A[i] <- scalars[i] A[i]
    truncated, shifted = linearCombinationsG1(curve, A, r, ends) / linearCombinationsG2   # what SameRatioMany pairs (Verify)

Points are numpy uint64 arrays of affine limbs (G1Affine / G2Affine layout), scalars and r fr.Elements in Montgomery limbs;
the linear combinations come back as Jacobian limbs. Results are new arrays; inputs are never modified. Precondition, as
for the reference's ScalarMultiplication: points lie in the r-torsion (Verify subgroup-checks first: ValidatePoints).
Pairings, hashing to G2 and the proof of knowledge stay with the caller. Errors raise ValueError with the library's text.
The *_device variants take raw device pointers (e.g. torch tensor.data_ptr()) and the stream that produced them; the
output pointer may equal the input pointer.
"""
import ctypes

import numpy as np

from . import _lib
from .curves import CURVES


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _curve(curve):
    return CURVES[curve] if isinstance(curve, str) else curve


def _gid(curve, which):
    return _lib.GROUP_IDS[(_curve(curve).name, which)]


def _aff_limbs(curve, which):
    return int(_lib.load().gmsm_affine_limbs(_gid(curve, which)))


def _check(rc):
    if rc:
        raise ValueError(_lib.last_error())


def _host_or_none(a):
    return _ptr(a) if a.size else None


def _points(curve, which, A):
    return np.ascontiguousarray(A, dtype=np.uint64).reshape(-1, _aff_limbs(curve, which))


def _batch_scale(curve, which, A, scalars):
    c = _curve(curve)
    pts = _points(c, which, A)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, c.fr_limbs)
    out = np.zeros_like(pts)
    _check(_lib.load().gmsm_batch_scale(_gid(c, which), _host_or_none(pts), None, pts.shape[0], _host_or_none(sc), None, sc.shape[0],
                                        None, _host_or_none(out), None))
    return out


def _update_monomials(curve, which, A, r):
    c = _curve(curve)
    pts = _points(c, which, A)
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(c.fr_limbs)
    out = np.zeros_like(pts)
    _check(_lib.load().gmsm_update_monomials(_gid(c, which), _host_or_none(pts), None, pts.shape[0], _ptr(r), None, _host_or_none(out), None))
    return out


def _linear_combinations(curve, which, A, r, ends, d_points=None, n=None, stream=0):
    c = _curve(curve)
    gid = _gid(c, which)
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(c.fr_limbs)
    ends = [int(e) for e in ends]
    cends = (ctypes.c_size_t * len(ends))(*ends) if ends else None
    jl = _aff_limbs(c, which) // 2 * 3
    t, s = np.zeros(jl, dtype=np.uint64), np.zeros(jl, dtype=np.uint64)
    if d_points is None:
        pts = _points(c, which, A)
        _check(_lib.load().gmsm_linear_combinations(gid, _host_or_none(pts), None, pts.shape[0], cends, len(ends), _ptr(r), None, _ptr(t), _ptr(s)))
    else:
        _check(_lib.load().gmsm_linear_combinations(gid, None, d_points, int(n), cends, len(ends), _ptr(r), stream or None, _ptr(t), _ptr(s)))
    return t, s


def UpdateMonomialsG1(curve, A, r):
    """mpcsetup.UpdateMonomialsG1: out[0] = A[0], out[i] = r^i A[i]; at least 2 points. r^i is made on the device."""
    return _update_monomials(curve, "g1", A, r)


def UpdateMonomialsG2(curve, A, r):
    """UpdateMonomialsG1 over G2Affine limbs."""
    return _update_monomials(curve, "g2", A, r)


def ScaleG1(curve, A, s):
    """out[i] = s A[i] (mpcsetup.UpdateValues on a []G1Affine)."""
    return _batch_scale(curve, "g1", A, np.ascontiguousarray(s, dtype=np.uint64).reshape(1, -1))


def ScaleG2(curve, A, s):
    """out[i] = s A[i] (mpcsetup.UpdateValues on a []G2Affine)."""
    return _batch_scale(curve, "g2", A, np.ascontiguousarray(s, dtype=np.uint64).reshape(1, -1))


def BatchScaleG1(curve, A, scalars):
    """out[i] = scalars[i] A[i]: len(scalars) must be len(A) (or 1: ScaleG1)."""
    return _batch_scale(curve, "g1", A, scalars)


def BatchScaleG2(curve, A, scalars):
    """out[i] = scalars[i] A[i] over G2Affine limbs."""
    return _batch_scale(curve, "g2", A, scalars)


def linearCombinationsG1(curve, A, r, ends):
    """linearCombinationsG1 (mpcsetup.go:396-447): (truncated, shifted) Jacobian limbs with, over powers[i] = r^i,
    truncated = sum r^i A[i] and shifted = sum r^i A[i+1] over every i that is not the last of its segment; `ends` are the
    running ends of the segments (each at least 2 long, the last one len(A))."""
    return _linear_combinations(curve, "g1", A, r, ends)


def linearCombinationsG2(curve, A, r, ends):
    """linearCombinationsG2 (mpcsetup.go:489-540): as linearCombinationsG1 over G2Affine limbs."""
    return _linear_combinations(curve, "g2", A, r, ends)


def batch_scale_device(curve, which, d_points, n, d_scalars, n_scalars, d_out, stream=0):
    """gmsm_batch_scale over device pointers: n points of group `which` ("g1" / "g2"), n_scalars = n or 1 fr.Elements."""
    _check(_lib.load().gmsm_batch_scale(_gid(curve, which), None, d_points, int(n), None, d_scalars, int(n_scalars), stream or None, None, d_out))


def update_monomials_device(curve, which, d_points, n, r, d_out, stream=0):
    """gmsm_update_monomials from device pointer d_points to d_out (may equal d_points); r is a host fr.Element."""
    c = _curve(curve)
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(c.fr_limbs)
    _check(_lib.load().gmsm_update_monomials(_gid(c, which), None, d_points, int(n), _ptr(r), stream or None, None, d_out))


def linear_combinations_device(curve, which, d_points, n, r, ends, stream=0):
    """gmsm_linear_combinations over n device points: (truncated, shifted) Jacobian limbs on the host."""
    return _linear_combinations(curve, which, None, r, ends, d_points=d_points, n=n, stream=stream)
