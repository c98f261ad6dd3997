"""fr/polynomial.MultiLin (ecc/<curve>/fr/polynomial/multilin.go) over libgmsm.so: the bookkeeping table of a multilinear
polynomial, 2^n Montgomery fr.Elements with X_1 the most significant bit of an index. Fold, Evaluate and Eq run on the device
(gmsm_multilin_fold / _evaluate / _eq, include/gmsm.h); Add, Sum and EvalEq are host big-int arithmetic, as small in the
reference. The *_device functions take raw device pointers and a stream."""
import ctypes

import numpy as np

from . import _lib
from .curves import CURVES


def _curve(curve):
    return CURVES[curve] if isinstance(curve, str) else curve


def _gid(curve):
    return _lib.GROUP_IDS[(_curve(curve).name, "g1")]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(rc):
    if rc:
        raise ValueError(_lib.last_error())


def _elems(c, x, count=None):
    a = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, c.fr_limbs)
    if count is not None and a.shape[0] != count:
        raise ValueError("expected %d elements, got %d" % (count, a.shape[0]))
    return a


def to_int(c, limbs):
    """the value of one element in Montgomery limbs"""
    m = sum(int(v) << (64 * i) for i, v in enumerate(np.asarray(limbs).reshape(-1)))
    return m * pow(c.fr_R, -1, c.r) % c.r


def from_int(c, v):
    m = int(v) % c.r * c.fr_R % c.r
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(c.fr_limbs)], dtype=np.uint64)


def fold_device(curve, d_a, length, r, stream=0):
    """(*MultiLin).Fold of the `length` elements at device pointer d_a, in place: the lower half is written."""
    c = _curve(curve)
    _check(_lib.load().gmsm_multilin_fold(_gid(c), None, d_a, int(length), _ptr(_elems(c, r, 1)), stream or None))


def evaluate_device(curve, d_m, length, coords, stream=0):
    """(MultiLin).Evaluate of the table at device pointer d_m, which is not modified; the value's limbs."""
    c = _curve(curve)
    co = _elems(c, coords)
    out = np.zeros(c.fr_limbs, dtype=np.uint64)
    _check(_lib.load().gmsm_multilin_evaluate(_gid(c), None, d_m, int(length), _ptr(co) if len(co) else None, len(co), stream or None, _ptr(out)))
    return out


def eq_device(curve, q, scale, d_out, accumulate=False, stream=0):
    """scale eq(q, .) written (or, accumulate, added) to the 2^len(q) elements at device pointer d_out."""
    c = _curve(curve)
    qq = _elems(c, q)
    _check(_lib.load().gmsm_multilin_eq(_gid(c), _ptr(qq) if len(qq) else None, len(qq), _ptr(_elems(c, scale, 1)), int(bool(accumulate)),
                                        stream or None, None, d_out))


class MultiLin:
    """polynomial.MultiLin: .values is the (len, fr_limbs) uint64 array of the table, len a power of two."""

    def __init__(self, curve, values):
        self.curve = _curve(curve)
        self.values = _elems(self.curve, values)

    def __len__(self):
        return self.values.shape[0]

    def NumVars(self):
        return (len(self) - 1).bit_length()  # bits.TrailingZeros of a power of two

    def Clone(self):
        return MultiLin(self.curve, self.values.copy())

    def Fold(self, r):
        """X_1 = r, in place; the table is then its lower half (a view: the upper half of the array stays as it was)."""
        c = self.curve
        _check(_lib.load().gmsm_multilin_fold(_gid(c), _ptr(self.values), None, len(self), _ptr(_elems(c, r, 1)), None))
        self.values = self.values[:len(self) // 2]

    def Evaluate(self, coordinates):
        c = self.curve
        co = _elems(c, coordinates)
        out = np.zeros(c.fr_limbs, dtype=np.uint64)
        _check(_lib.load().gmsm_multilin_evaluate(_gid(c), _ptr(self.values), None, len(self), _ptr(co) if len(co) else None, len(co), None, _ptr(out)))
        return out

    def Eq(self, q):
        """the table of Eq(q_1 .. q_n, *) x m[0]; len(m) must be 2^len(q)"""
        c = self.curve
        qq = _elems(c, q)
        if len(self) != 1 << len(qq):
            raise ValueError("destination must have size 2 raised to the size of source")
        scale = self.values[0].copy()
        _check(_lib.load().gmsm_multilin_eq(_gid(c), _ptr(qq) if len(qq) else None, len(qq), _ptr(scale), 0, None, _ptr(self.values), None))

    def Add(self, left, right):
        if not (len(left) == len(right) == len(self)):
            raise ValueError("left, right and destination must have the right size")
        c = self.curve
        for i in range(len(self)):
            self.values[i] = from_int(c, to_int(c, left.values[i]) + to_int(c, right.values[i]))

    def Sum(self):
        c = self.curve
        return from_int(c, sum(to_int(c, v) for v in self.values))


def EvalEq(curve, q, h):
    """Eq(q, h) = prod_i (1 + 2 q_i h_i - q_i - h_i) (multilin.go:140-160), host arithmetic; the value's limbs."""
    c = _curve(curve)
    res = 1
    for a, b in zip(_elems(c, q), _elems(c, h)):
        x, y = to_int(c, a), to_int(c, b)
        res = res * (1 + 2 * x * y - x - y) % c.r
    return from_int(c, res)
