"""Host-side mirror of the prover half of gnark-crypto's shplonk package on top of the C ABI (include/gmsm.h,
gmsm_shplonk_open_w / gmsm_shplonk_open_wprime): polynomial i is opened on its own set of points, the division chains, the
accumulation and the two commitments run on the device over resident bases.

Keeps the reference's names and meaning (ecc/bn254/shplonk/shplonk.go:44-172):

    W, WPrime, claimed = BatchOpen(polynomials, points, gamma, z_of_W, rb)   # BatchOpen after the challenges
    claimed, w, W = OpenW(polynomials, points, gamma, rb)                    # :97-121: w = sum_i gamma^i Z_(T\\S_i)(f_i - r_i) / Z_T
    WPrime = OpenWPrime(polynomials, points, claimed, gamma, w, z, rb)       # :132-166: Commit(L / (X - z))

The Fiat-Shamir transcript stays with the caller, as gamma does in kzg.BatchOpenSinglePoint: gamma is an argument and z
comes from the callable z_of_W, which receives the affine W (deriveChallenge("z", nil, {W}, fs), shplonk.go:127).

Polynomials, points and field elements are numpy uint64 arrays in the layout of []fr.Element (Montgomery limbs), lowest
degree first; points[i] is the set S_i of polynomial i, claimed values come back as one array per polynomial in the same
order; W and WPrime are affine commitments (G1Affine limbs); w has max_i len(f_i) coefficients, zero above its degree.
Inputs are never modified. Errors raise ValueError with the library's text. Unlike the reference, two equal points
inside one set are refused (its interpolate inverts zero there and returns a meaningless proof without an error); equal
points in different sets are fine. The *_device variants take raw device pointers (e.g. torch tensor.data_ptr()) and the
stream that produced them.
"""
import ctypes

import numpy as np

from . import _lib
from .kzg import _affine, _check, _concat, _elem, _host_or_none, _ptr

ERR_NB_POINTS = "number of digests should be equal to the number of points"  # ErrInvalidNumberOfPoints, shplonk.go:21


def _point_sets(curve, points):
    nl = curve.fr_limbs
    sets = [np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, nl) for s in points]
    npoints = (ctypes.c_size_t * len(sets))(*[s.shape[0] for s in sets])
    flat = np.concatenate(sets) if sets else np.zeros((0, nl), dtype=np.uint64)
    return np.ascontiguousarray(flat), npoints


def _split(flat, npoints):
    out, at = [], 0
    for m in npoints:
        out.append(flat[at:at + m].copy())
        at += m
    return out


def _check_counts(polynomials, points):
    if len(polynomials) != len(points):
        raise ValueError(ERR_NB_POINTS)


def OpenW(polynomials, points, gamma, rb):
    """The first half of BatchOpen (shplonk.go:97-121) after the challenge gamma: returns (claimed values, w, W affine)
    with claimed[i][j] = f_i(points[i][j]) and W = Commit(w)."""
    _check_counts(polynomials, points)
    g = rb.group
    flat, lens = _concat(g.curve, polynomials)
    pts, npoints = _point_sets(g.curve, points)
    gamma = _elem(g.curve, gamma)
    claimed = np.zeros_like(pts)
    w = np.zeros((max(list(lens), default=0), g.fr_limbs), dtype=np.uint64)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_shplonk_open_w(rb.handle, _host_or_none(flat), None, lens, len(lens), _host_or_none(pts), npoints,
                                           _ptr(gamma), None, _host_or_none(claimed), _host_or_none(w), None, _ptr(jac)))
    return _split(claimed, list(npoints)), w, _affine(rb, jac)


def open_w_device(d_polys, lens, points, gamma, rb, d_out_w, stream=0):
    """OpenW over k polynomials concatenated at device pointer d_polys (lens[i] coefficients each, produced on `stream`);
    w goes to device pointer d_out_w (max(lens) elements). Returns (claimed values, W affine)."""
    _check_counts(lens, points)
    g = rb.group
    clens = (ctypes.c_size_t * len(lens))(*[int(x) for x in lens])
    pts, npoints = _point_sets(g.curve, points)
    gamma = _elem(g.curve, gamma)
    claimed = np.zeros_like(pts)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_shplonk_open_w(rb.handle, None, d_polys, clens, len(lens), _host_or_none(pts), npoints, _ptr(gamma),
                                           stream or None, _host_or_none(claimed), None, d_out_w, _ptr(jac)))
    return _split(claimed, list(npoints)), _affine(rb, jac)


def OpenWPrime(polynomials, points, claimed, gamma, w, z, rb):
    """The second half of BatchOpen (shplonk.go:132-166) after the challenge z: WPrime = Commit(L / (X - z)) with
    L = sum_i gamma^i Z_(T\\S_i)(z) (f_i - r_i(z)) - Z_T(z) w, as an affine point."""
    _check_counts(polynomials, points)
    g = rb.group
    flat, lens = _concat(g.curve, polynomials)
    pts, npoints = _point_sets(g.curve, points)
    vals, _ = _point_sets(g.curve, claimed)
    if vals.shape != pts.shape:
        raise ValueError(ERR_NB_POINTS)
    gamma, z = _elem(g.curve, gamma), _elem(g.curve, z)
    w = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, g.fr_limbs)
    if w.shape[0] != max(list(lens), default=0):
        raise ValueError("shplonk: w must have max(len(polynomials[i])) coefficients")
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_shplonk_open_wprime(rb.handle, _host_or_none(flat), None, lens, len(lens), _host_or_none(pts), npoints,
                                                _host_or_none(vals), _ptr(gamma), _host_or_none(w), None, _ptr(z), None, _ptr(jac)))
    return _affine(rb, jac)


def open_wprime_device(d_polys, lens, points, claimed, gamma, d_w, z, rb, stream=0):
    """OpenWPrime over device polynomials (as open_w_device) and the device vector d_w that open_w_device wrote."""
    _check_counts(lens, points)
    g = rb.group
    clens = (ctypes.c_size_t * len(lens))(*[int(x) for x in lens])
    pts, npoints = _point_sets(g.curve, points)
    vals, _ = _point_sets(g.curve, claimed)
    if vals.shape != pts.shape:
        raise ValueError(ERR_NB_POINTS)
    gamma, z = _elem(g.curve, gamma), _elem(g.curve, z)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_shplonk_open_wprime(rb.handle, None, d_polys, clens, len(lens), _host_or_none(pts), npoints,
                                                _host_or_none(vals), _ptr(gamma), None, d_w, _ptr(z), stream or None, _ptr(jac)))
    return _affine(rb, jac)


def BatchOpen(polynomials, points, gamma, z_of_W, rb):
    """shplonk.BatchOpen after the Fiat-Shamir challenges: returns (W affine, WPrime affine, claimed values).
    z_of_W(W) returns the challenge z for the affine commitment W (the transcript stays with the caller)."""
    claimed, w, W = OpenW(polynomials, points, gamma, rb)
    z = z_of_W(W)
    return W, OpenWPrime(polynomials, points, claimed, gamma, w, z, rb), claimed
