"""Host-side mirror of the prover half of gnark-crypto's fflonk package on top of the C ABI (include/gmsm.h, gmsm_fflonk_*):
packs of polynomials are folded, committed and opened on the device over resident bases.

Keeps the reference's names and meaning (ecc/bn254/fflonk/fflonk.go:41-141):

    t = NextDivisor(curve, n)                                          # getNextDivisorRMinusOne (:234-252)
    folded = Fold(curve, pack)                                         # Fold (:52-71): sum_(j<t) P_j(X^t) X^j
    digest = FoldAndCommit(pack, rb)                                   # FoldAndCommit (:43-47)
    W, WPrime, folded_claimed, claimed = BatchOpen(packs, points, gamma, z_of_W, rb)   # BatchOpen (:77-141) after the challenges
    claimed, folded_claimed, w, W = OpenW(packs, points, gamma, rb)    # its first half: shplonk's w over the folded polynomials
    WPrime = OpenWPrime(packs, points, folded_claimed, gamma, w, z, rb)  # its second half: Commit(L / (X - z))

The Fiat-Shamir transcript stays with the caller, as in gnark-crypto_amd/shplonk.py: gamma is an argument and z comes from
the callable z_of_W, which receives the affine W.

packs[i] is a list of polynomials, points[i] the BASE points of pack i (the library extends each to its orbit under the
t_i-th roots of one). Polynomials, points and field elements are numpy uint64 arrays in the layout of []fr.Element
(Montgomery limbs), lowest degree first; an empty member of a non-empty pack is the zero polynomial. claimed[i] has shape
(t_i, len(points[i]), limbs) - OpeningProof.ClaimedValues[i][j][k], rows past the pack's size zero - and folded_claimed[i]
shape (t_i len(points[i]), limbs) - SOpeningProof.ClaimedValues[i][k t_i + l]; W, WPrime and digests are affine
commitments (G1Affine limbs); w has max_i t_i max_j len(packs[i][j]) coefficients, zero above its degree. Inputs are
never modified. Errors raise ValueError with the library's text. Unlike the reference, two equal points in an extended
set (z_a^t = z_b^t, or z = 0 with t > 1) are refused: shplonk's interpolate inverts zero there. The *_device variants take
raw device pointers (e.g. torch tensor.data_ptr()) and the stream that produced them.
"""
import ctypes

import numpy as np

from . import _lib
from .kzg import _affine, _check, _concat, _curve, _elem, _gid, _host_or_none, _ptr
from .shplonk import _point_sets

ERR_NB_PACKS = "the number of packs of polynomials should be the same as the number of pack of points"  # ErrNbPolynomialsNbPoints


def NextDivisor(curve, n):
    """getNextDivisorRMinusOne(n): the smallest divisor of r - 1 that is >= n (ValueError when 100 trials find none)."""
    t = ctypes.c_size_t(0)
    _check(_lib.load().gmsm_fflonk_next_divisor(_gid(curve), int(n), ctypes.byref(t)))
    return int(t.value)


def _divisor_or_zero(curve, n):
    """t for sizing the outputs; 0 where the library is going to refuse the call with its own text"""
    t = ctypes.c_size_t(0)
    return int(t.value) if n > 0 and _lib.load().gmsm_fflonk_next_divisor(_gid(curve), int(n), ctypes.byref(t)) == 0 else 0


def _sizes(v):
    return (ctypes.c_size_t * len(v))(*[int(x) for x in v])


def _out(rows, nl):
    """an output of `rows` elements with a valid pointer even when rows == 0 (the library then refuses the call itself)"""
    return np.zeros((max(rows, 1), nl), dtype=np.uint64)


def _layout(curve, pack_sizes, lens, npoints):
    """t_i, the rows of both claimed vectors per pack, the length of w"""
    ts = [_divisor_or_zero(curve, c) for c in pack_sizes]
    wlen, at = 0, 0
    for t, c in zip(ts, pack_sizes):
        wlen = max(wlen, t * max(list(lens[at:at + c]), default=0))
        at += c
    return ts, [t * m for t, m in zip(ts, npoints)], wlen


def _split_claimed(claimed, folded, ts, npoints, nl):
    out_c, out_f, at = [], [], 0
    for t, m in zip(ts, npoints):
        out_c.append(claimed[at:at + t * m].reshape(t, m, nl).copy())
        out_f.append(folded[at:at + t * m].copy())
        at += t * m
    return out_c, out_f


def _flatten(curve, packs):
    flat, lens = _concat(curve, [p for pack in packs for p in pack])
    return flat, lens, [len(pack) for pack in packs]


def Fold(curve, pack):
    """Fold(pack): t max_j len(pack[j]) coefficients, out[j t + i] = pack[i][j]."""
    c = _curve(curve)
    flat, lens = _concat(c, pack)
    t = _divisor_or_zero(c, len(lens))
    n = t * max(list(lens), default=0)
    out = _out(n, c.fr_limbs)
    _check(_lib.load().gmsm_fflonk_fold(_gid(c), _host_or_none(flat), None, lens, len(lens), None, _ptr(out), None))
    return out[:n]


def fold_device(curve, d_polys, lens, d_out, stream=0):
    """Fold of one pack concatenated at device pointer d_polys (lens[j] coefficients each, produced on `stream`) into
    device pointer d_out (NextDivisor(len(lens)) max(lens) elements)."""
    _check(_lib.load().gmsm_fflonk_fold(_gid(curve), None, d_polys, _sizes(lens), len(lens), stream or None, None, d_out))


def FoldAndCommit(pack, rb):
    """FoldAndCommit(pack, pk) with pk's G1 registered as rb: the affine digest of Fold(pack)."""
    g = rb.group
    flat, lens = _concat(g.curve, pack)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_fflonk_fold_commit(rb.handle, _host_or_none(flat), None, lens, len(lens), None, None, _ptr(jac)))
    return _affine(rb, jac)


def fold_commit_device(d_polys, lens, rb, d_out_folded=None, stream=0):
    """FoldAndCommit over a device pack (as fold_device); the folded polynomial also goes to d_out_folded when given."""
    jac = np.zeros(rb.group.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_fflonk_fold_commit(rb.handle, None, d_polys, _sizes(lens), len(lens), stream or None, d_out_folded, _ptr(jac)))
    return _affine(rb, jac)


def _check_counts(packs, points):
    if len(packs) != len(points):
        raise ValueError(ERR_NB_PACKS)


def _open_w(rb, flat_ptr, d_polys, lens, pack_sizes, points, gamma, w_rows_out, d_out_w, stream):
    g = rb.group
    nl = g.fr_limbs
    pts, npoints = _point_sets(g.curve, points)
    ts, rows, wlen = _layout(g.curve, pack_sizes, lens, list(npoints))
    gamma = _elem(g.curve, gamma)
    claimed, folded = _out(sum(rows), nl), _out(sum(rows), nl)
    w = _out(wlen, nl) if w_rows_out else None
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_fflonk_open_w(rb.handle, flat_ptr, d_polys, _sizes(lens), _sizes(pack_sizes), len(pack_sizes), _host_or_none(pts),
                                          npoints, _ptr(gamma), stream or None, _ptr(claimed), _ptr(folded), _ptr(w) if w_rows_out else None,
                                          d_out_w, _ptr(jac)))
    c, f = _split_claimed(claimed, folded, ts, list(npoints), nl)
    return c, f, (w[:wlen] if w_rows_out else None), _affine(rb, jac)


def OpenW(packs, points, gamma, rb):
    """The first half of BatchOpen after the challenge gamma: returns (claimed, folded_claimed, w, W affine)."""
    _check_counts(packs, points)
    flat, lens, pack_sizes = _flatten(rb.group.curve, packs)
    return _open_w(rb, _host_or_none(flat), None, list(lens), pack_sizes, points, gamma, True, None, 0)


def open_w_device(d_polys, lens, pack_sizes, points, gamma, rb, d_out_w, stream=0):
    """OpenW over packs concatenated at device pointer d_polys (lens[j] coefficients per polynomial, pack_sizes[i]
    polynomials per pack, produced on `stream`); w goes to device pointer d_out_w. Returns (claimed, folded_claimed, W)."""
    _check_counts(pack_sizes, points)
    c, f, _, W = _open_w(rb, None, d_polys, list(lens), list(pack_sizes), points, gamma, False, d_out_w, stream)
    return c, f, W


def _open_wprime(rb, flat_ptr, d_polys, lens, pack_sizes, points, folded_claimed, gamma, w_ptr, d_w, z, stream):
    g = rb.group
    pts, npoints = _point_sets(g.curve, points)
    vals, nvals = _point_sets(g.curve, folded_claimed)
    ts, rows, _ = _layout(g.curve, pack_sizes, lens, list(npoints))
    if all(ts) and list(nvals) != rows:
        raise ValueError("fflonk: folded_claimed[i] must hold t_i len(points[i]) values")
    gamma, z = _elem(g.curve, gamma), _elem(g.curve, z)
    jac = np.zeros(g.jac_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_fflonk_open_wprime(rb.handle, flat_ptr, d_polys, _sizes(lens), _sizes(pack_sizes), len(pack_sizes),
                                               _host_or_none(pts), npoints, _ptr(vals) if vals.size else _ptr(_out(0, g.fr_limbs)), _ptr(gamma),
                                               w_ptr, d_w, _ptr(z), stream or None, _ptr(jac)))
    return _affine(rb, jac)


def OpenWPrime(packs, points, folded_claimed, gamma, w, z, rb):
    """The second half of BatchOpen after the challenge z: WPrime = Commit(L / (X - z)) as an affine point."""
    _check_counts(packs, points)
    g = rb.group
    flat, lens, pack_sizes = _flatten(g.curve, packs)
    w = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, g.fr_limbs)
    _, _, wlen = _layout(g.curve, pack_sizes, list(lens), [0] * len(pack_sizes))
    if w.shape[0] != wlen:
        raise ValueError("fflonk: w must have max_i t_i max_j len(packs[i][j]) coefficients")
    wbuf = w if w.size else _out(0, g.fr_limbs)
    return _open_wprime(rb, _host_or_none(flat), None, list(lens), pack_sizes, points, folded_claimed, gamma, _ptr(wbuf), None, z, 0)


def open_wprime_device(d_polys, lens, pack_sizes, points, folded_claimed, gamma, d_w, z, rb, stream=0):
    """OpenWPrime over device packs (as open_w_device) and the device vector d_w that open_w_device wrote."""
    _check_counts(pack_sizes, points)
    return _open_wprime(rb, None, d_polys, list(lens), list(pack_sizes), points, folded_claimed, gamma, None, d_w, z, stream)


def BatchOpen(packs, points, gamma, z_of_W, rb):
    """fflonk.BatchOpen after the Fiat-Shamir challenges: returns (W affine, WPrime affine, folded_claimed, claimed).
    z_of_W(W) returns the challenge z for the affine commitment W (the transcript stays with the caller)."""
    claimed, folded_claimed, w, W = OpenW(packs, points, gamma, rb)
    z = z_of_W(W)
    return W, OpenWPrime(packs, points, folded_claimed, gamma, w, z, rb), folded_claimed, claimed
