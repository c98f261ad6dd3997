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

with to_basis_device, evaluate_device and divide_by_x_minus_one_device over raw device pointers.

iop.Evaluate(f Expression, r, form, x...) (expressions.go:26-73) over gmsm_iop_evaluate_expression. A closure cannot run on
the device; an expression is a fixed sequence of field operations, so f is TRACED once with symbols into a straight-line
program (Program), which one kernel interprets, one index per lane:

    h = Evaluate(lambda i, a, b, c: a * a * b + c - a * a * a, None, Form(LagrangeCoset, Regular), pa, pb, pc)
    z = Evaluate(lambda i, a: a * i.point(), None, form, pa, domain=d)   # i.point() = w^i, the only use of i there is

with evaluate_expression_device over raw device pointers (one per input: resident polynomials are not concatenated).
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


# ---- iop.Evaluate (expressions.go:26-73) over gmsm_iop_evaluate_expression
# the opcodes and limits of include/gmsm.h (GMSM_EXPR_*)
EXPR_INPUT, EXPR_CONST, EXPR_POINT, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG = 1, 2, 3, 4, 5, 6, 7
EXPR_MAX_REGS, EXPR_MAX_INSNS, EXPR_MAX_INPUTS, EXPR_MAX_CONSTS = 16, 4096, 64, 256
ErrNoInput = "need at lest one input"  # the reference's text, typo included (expressions.go:39)

Code = namedtuple("Code", ["words", "consts", "has_point"])  # uint32 instruction words, (n_consts, fr_limbs) Montgomery limbs


class Symbol:
    """A value of a Program: the result of one instruction. + - * and unary - make new symbols; a Python int or an array of
    Montgomery limbs on either side becomes a constant."""

    __slots__ = ("program", "id")
    __array_ufunc__ = None  # numpy leaves `array * symbol` to __rmul__

    def __init__(self, program, id_):
        self.program, self.id = program, id_

    def _other(self, o):
        if isinstance(o, Symbol):
            if o.program is not self.program:
                raise ValueError("symbols of two programs")
            return o
        return self.program.const(o)

    def __add__(self, o):
        return self.program._emit(EXPR_ADD, self, self._other(o))

    def __radd__(self, o):
        return self.program._emit(EXPR_ADD, self._other(o), self)

    def __sub__(self, o):
        return self.program._emit(EXPR_SUB, self, self._other(o))

    def __rsub__(self, o):
        return self.program._emit(EXPR_SUB, self._other(o), self)

    def __mul__(self, o):
        return self.program._emit(EXPR_MUL, self, self._other(o))

    def __rmul__(self, o):
        return self.program._emit(EXPR_MUL, self._other(o), self)

    def __neg__(self):
        return self.program._emit(EXPR_NEG, self)


class IndexSymbol:
    """The closure's argument i while it is traced: its only operation is point() = w^i, w = fft.Generator(len)."""

    def __init__(self, program):
        self.program = program

    def point(self):
        return self.program.point()


class Program:
    """Builder of a straight-line program. input(j), const(value) and point() give symbols, the operators combine them;
    build(result) emits the instructions that result needs, in the order they were made (evaluation order; an input, constant
    or point just before its first use), with registers allocated by liveness: a register is free again after the last use of its symbol, so a symbol used twice is computed once
    and a chain of products needs two registers. More than 16 live registers raise ValueError."""

    def __init__(self, curve):
        self.curve = _curve(curve)
        self.nodes = []  # (op, a, b): a, b symbol ids for the arithmetic, an input / constant index for INPUT / CONST
        self.consts, self._const_ids, self._input_ids, self._point = [], {}, {}, None

    def _node(self, op, a=0, b=0):
        self.nodes.append((op, a, b))
        return Symbol(self, len(self.nodes) - 1)

    def _emit(self, op, a, b=None):
        return self._node(op, a.id, a.id if b is None else b.id)

    def input(self, j):
        j = int(j)
        if not 0 <= j < EXPR_MAX_INPUTS:
            raise ValueError("input %d is outside [0, %d)" % (j, EXPR_MAX_INPUTS))
        if j not in self._input_ids:
            self._input_ids[j] = self._node(EXPR_INPUT, j)
        return self._input_ids[j]

    def const(self, value):
        """A Python int is a true value (reduced mod r); anything else is one element in Montgomery limbs."""
        c = self.curve
        if isinstance(value, (int, np.integer)):
            m = int(value) % c.r * c.fr_R % c.r
            limbs = tuple((m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(c.fr_limbs))
        else:
            limbs = tuple(int(v) for v in _elem(c, value))
        if limbs not in self._const_ids:
            if len(self.consts) == EXPR_MAX_CONSTS:
                raise ValueError("more than %d constants" % EXPR_MAX_CONSTS)
            self.consts.append(limbs)
            self._const_ids[limbs] = self._node(EXPR_CONST, len(self.consts) - 1)
        return self._const_ids[limbs]

    def point(self):
        if self._point is None:
            self._point = self._node(EXPR_POINT)
        return self._point

    def index(self):
        return IndexSymbol(self)

    def build(self, result):
        if not isinstance(result, Symbol):
            result = self.const(result)
        if result.program is not self:
            raise ValueError("the result is a symbol of another program")
        arith = (EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG)
        operands = lambda n: () if n[0] not in arith else (n[1],) if n[0] == EXPR_NEG else (n[1], n[2])
        needed, stack = set(), [result.id]
        while stack:
            k = stack.pop()
            if k not in needed:
                needed.add(k)
                stack.extend(operands(self.nodes[k]))
        # creation order is evaluation order: operands exist before their users. A leaf (INPUT, CONST, POINT) is emitted just
        # before its first user, not where it was made: the m inputs of a traced function are not all live from the start
        order, placed = [], set()
        for k in sorted(needed):
            if self.nodes[k][0] in arith:
                for o in operands(self.nodes[k]):
                    if self.nodes[o][0] not in arith and o not in placed:
                        placed.add(o)
                        order.append(o)
                order.append(k)
        if not order:
            order = [result.id]  # the result is a leaf
        if len(order) > EXPR_MAX_INSNS:
            raise ValueError("the program has %d instructions, more than %d" % (len(order), EXPR_MAX_INSNS))
        last_use = {}
        for k in order:
            for o in operands(self.nodes[k]):
                last_use[o] = k
        free, reg, words, used_consts, const_at = list(range(EXPR_MAX_REGS - 1, -1, -1)), {}, [], [], {}
        for k in order:
            op, a, b = self.nodes[k]
            ops = operands(self.nodes[k])
            ra, rb = (reg[ops[0]] if ops else a), (reg[ops[1]] if len(ops) > 1 else 0)
            if op == EXPR_CONST:  # only the constants the result needs travel
                if a not in const_at:
                    const_at[a] = len(used_consts)
                    used_consts.append(self.consts[a])
                ra = const_at[a]
            for o in set(ops):  # the destination may be an operand's register: the lane reads both before it writes
                if last_use[o] == k:
                    free.append(reg.pop(o))
            if not free:
                raise ValueError("more than %d registers are live at instruction %d" % (EXPR_MAX_REGS, len(words)))
            free.sort(reverse=True)
            reg[k] = free.pop()  # the lowest free register: the kernel's register file is sized by the highest one used
            words.append(op | reg[k] << 8 | ra << 16 | rb << 24)
        consts = np.array(used_consts, dtype=np.uint64).reshape(-1, self.curve.fr_limbs)
        return Code(np.array(words, dtype=np.uint32), consts, any(self.nodes[k][0] == EXPR_POINT for k in order))


def trace(curve, f, m):
    """f(i, x_0, .., x_(m-1)) called ONCE with symbols: the Code of its result."""
    p = Program(curve)
    return p.build(f(p.index(), *[p.input(j) for j in range(m)]))


def _expression_call(c, code, domain, polys, d_polys, m, length, sizes, shifts, layouts, out_layout, stream, out, d_out):
    words = np.ascontiguousarray(code[0], dtype=np.uint32).reshape(-1)
    consts = np.ascontiguousarray(code[1], dtype=np.uint64).reshape(-1, c.fr_limbs)
    sz = np.ascontiguousarray([int(v) for v in sizes], dtype=np.uintp)
    sh = np.ascontiguousarray([int(v) for v in shifts], dtype=np.int64)
    lay = _layouts(layouts)
    if not (len(sz) == len(sh) == len(lay) == m):
        raise ValueError("sizes, shifts and layouts must have one entry per input")
    ptrs = None if m == 0 else (ctypes.c_void_p * m)(*[int(v) for v in (polys if polys is not None else d_polys)])
    _check(_lib.load().gmsm_iop_evaluate_expression(
        _gid(c), domain.handle if domain is not None else 0, words.ctypes.data_as(_u32p), len(words), _ptr(consts) if len(consts) else None,
        len(consts), ptrs if polys is not None else None, ptrs if polys is None else None, m, int(length),
        sz.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), sh.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), lay.ctypes.data_as(_u32p),
        int(out_layout), stream or None, out, d_out))


def evaluate_expression_device(curve, program, d_polys, length, sizes, shifts, layouts, out_layout, d_out, domain=None, stream=0):
    """The program (a Code, or its (words, consts)) over the m = len(d_polys) polynomials of `length` elements at the device
    pointers d_polys, produced on `stream`, into d_out - which may be one of them when layout and offset allow (include/gmsm.h).
    domain: the fft.Domain of cardinality `length`, needed by a program with point()."""
    _expression_call(_curve(curve), program, domain, None, list(d_polys), len(d_polys), length, sizes, shifts, layouts, out_layout, stream, None,
                     d_out)


def Evaluate(f, r, form, *x, domain=None):
    """iop.Evaluate (expressions.go:26-73): f(i, x_0, .., x_(m-1)), an ordinary callable over + - * and unary -, applied to
    the m polynomials index by index on the device; i.point() is w^i. r: None, or the array the result is written to (it may
    be the coefficients of an input of the result's layout and shift 0). The result has x[0]'s size and shift 0."""
    if not x:
        raise ValueError(ErrNoInput)
    c = x[0].curve
    n = x[0].coefficients.shape[0]
    for p in x[1:]:
        if p.coefficients.shape[0] != n:
            raise ValueError(ErrInconsistentSize)
    if r is None:
        r = np.zeros((n, c.fr_limbs), dtype=np.uint64)
    elif not (isinstance(r, np.ndarray) and r.dtype == np.uint64 and r.flags.c_contiguous and r.size == n * c.fr_limbs):
        raise ValueError(ErrInconsistentSize)
    code = trace(c, f, len(x))
    own = None
    if code.has_point and domain is None and n:
        domain = own = fft.NewDomain(c, n)  # refused there when n is no power of two within the field's 2-adicity
    try:
        if n:
            _expression_call(c, code, domain if code.has_point else None, [p.coefficients.ctypes.data for p in x], None, len(x), n,
                             [p.size for p in x], [p.shift for p in x], [p.Layout for p in x], form[1], 0, _ptr(r), None)
    finally:
        if own is not None:
            own.release()
    res = Polynomial(c, r, form)
    res.size, res.shift = x[0].size, 0
    return res
