"""iop.Evaluate on the device (gnark-crypto_amd/iop.py over gmsm_iop_evaluate_expression): every output limb for limb against
the big-int model of tests/iop_expr_model.py (the reference's loop, pinned to the tracer by tests/test_iop_expr_model.py):
  - the reference's TestEvaluate through iop.Evaluate for the three scalar fields: size 64, the three layout mixes, both
    output layouts
  - the TestQuotient expression x1^2 x2 + x3 - x1^3 on random inputs at len 1, 2, 8, 63, 64, 65, 256, 257, 2^11 and 2^11 + 5:
    across a wave, a workgroup and several workgroups, the odd ones with a ragged last workgroup (Regular layouts only there).
    The kernel has no loop over indices - a lane owns one index and the grid is not capped - so there is no second trip to force
  - m = 5 at len 2^11 with mixed layouts, sizes (2^11, 2^9, 2^9, 2^11, 2^10), shifts (0, 1, 3, 0, 5), output BitReverse: host
    pointers, and device pointers on a non-default torch stream; inputs unchanged
  - POINT: x0 (c w^i) + x1 at len 1, 2, 8, 2^11; refused without a domain and with a domain of another cardinality
  - register pressure for BN254 and BW6-761 (48-byte elements: the largest register file, the smallest workgroup): all 16
    registers live, and a chain of 4096 instructions
  - in place: the output is input j (same layout, offset 0); a layout mismatch, a non-zero offset and a pointer 16 bytes into an
    input are refused and nothing is written
  - the reference's TestDivideByXMinusOne at n = 8 and n = 2^9 resident throughout: to_basis_device to the big coset, the
    expression, divide_by_x_minus_one_device; the result is the model's quotient
  - four threads, each with its own program on its own stream
  - with gmsm_set_profiling(1) the kernel's time goes to stage slot 0"""
import ctypes
import threading

import numpy as np
import pytest

import iop_expr_model as E
import iop_model as M
import iop_poly_model as P
from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
CAN, LAG, COS = P.CANONICAL, P.LAGRANGE, P.LAGRANGE_COSET
REG, REV = P.REGULAR, P.BIT_REVERSE
_VEC = {}


def vector(gm, curve, tag, count):
    """count random elements, made once per (curve, tag, count): (limbs, read-only; true values)"""
    key = (curve, tag, count)
    if key not in _VEC:
        c = gm.CURVES[curve]
        limbs = random_field_limbs(rng_for(0x10E0, CURVES.index(curve), tag, count), c.r, c.fr_limbs, count)
        limbs.setflags(write=False)
        _VEC[key] = (limbs, M.from_limbs(c, limbs))
    return _VEC[key]


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda() * 1  # produced by a kernel on the current stream


def download(c, t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs)


def inputs(gm, curve, n, layouts, sizes=None, shifts=None, tag0=0):
    """m random polynomials of n elements as (mirror polynomials, model polynomials) with the same layout, size and shift"""
    mirror, model = [], []
    for j, layout in enumerate(layouts):
        limbs, vals = vector(gm, curve, tag0 + j, n)
        mp = P.Polynomial(vals, LAG, layout)
        p = gm.iop.NewPolynomial(curve, limbs.copy(), gm.iop.Form(LAG, layout))
        if sizes:
            mp.size = sizes[j]
            p.SetSize(sizes[j])
        if shifts:
            mp.shift = shifts[j]
            p.Shift(shifts[j])
        mirror.append(p), model.append(mp)
    return mirror, model


def run_device(gm, curve, code, polys, out_layout, domain=None, out_index=None):
    """the resident form on a non-default torch stream: every input its own allocation; out_index: in place on that input.
    Returns (the output, the inputs as they are after the call)"""
    import torch
    c = gm.CURVES[curve]
    n = polys[0].coefficients.shape[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ts = [upload(p.coefficients) for p in polys]
        out = ts[out_index] if out_index is not None else upload(np.full((n, c.fr_limbs), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
        gm.iop.evaluate_expression_device(curve, code, [t.data_ptr() for t in ts], n, [p.size for p in polys], [p.shift for p in polys],
                                          [p.Layout for p in polys], out_layout, out.data_ptr(), domain=domain, stream=s.cuda_stream)
    s.synchronize()
    return download(c, out), [download(c, t) for t in ts]


# ------------------------------------------------------------------ the reference's TestEvaluate
@pytest.mark.parametrize("curve", CURVES)
def test_reference_test_evaluate(gm, curve):
    c, iop = gm.CURVES[curve], gm.iop
    size = 64
    expected = [3 * (i + 1) for i in range(size)]
    want = {REG: M.to_limbs(c, expected), REV: M.to_limbs(c, [expected[M.bit_reverse_index(i, size)] for i in range(size)])}
    for mix in ([REG, REG, REG], [REV, REG, REG], [REV, REV, REV]):
        polys = []
        for k, layout in enumerate(mix):
            vals = [i + k for i in range(size)]
            stored = vals if layout == REG else [vals[M.bit_reverse_index(i, size)] for i in range(size)]
            polys.append(iop.NewPolynomial(curve, M.to_limbs(c, stored), iop.Form(CAN, layout)))
        for out_layout in (REG, REV):
            res = iop.Evaluate(E.sum_expression, None, iop.Form(CAN, out_layout), *polys)
            assert (res.Basis, res.Layout, res.Size(), res.shift) == (CAN, out_layout, size, 0)
            assert (res.Coefficients() == want[out_layout]).all(), (mix, out_layout)


# ------------------------------------------------------------------ the TestQuotient expression across launch shapes
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_expression_lengths(gm, curve):
    c, iop = gm.CURVES[curve], gm.iop
    code = iop.trace(curve, E.quotient_expression, 3)
    for k, n in enumerate([1, 2, 8, 63, 64, 65, 256, 257, 1 << 11, (1 << 11) + 5]):
        pow2 = n & (n - 1) == 0
        layouts = [REG, REV, REG] if pow2 else [REG] * 3
        out_layout = REV if pow2 and k % 2 else REG
        mirror, model = inputs(gm, curve, n, layouts)
        want = M.to_limbs(c, E.evaluate(c, E.quotient_expression, (COS, out_layout), model).coefficients)
        res = iop.Evaluate(E.quotient_expression, None, iop.Form(COS, out_layout), *mirror)  # host pointers
        assert (res.Coefficients() == want).all(), n
        got, after = run_device(gm, curve, code, mirror, out_layout)
        assert (got == want).all(), n
        for p, t in zip(mirror, after):
            assert (t == p.coefficients).all()


# ------------------------------------------------------------------ m = 5, sizes and shifts
def five(i, a, b, c_, d, e):
    return a * b + c_ * d - e * 0x1234567890ABCDEF1234567890ABCDEF + a


@pytest.mark.parametrize("curve", CURVES)
def test_five_inputs_sizes_and_shifts(gm, curve):
    c, iop = gm.CURVES[curve], gm.iop
    n = 1 << 11
    layouts, sizes, shifts = [REG, REV, REV, REG, REV], [1 << 11, 1 << 9, 1 << 9, 1 << 11, 1 << 10], [0, 1, 3, 0, 5]
    mirror, model = inputs(gm, curve, n, layouts, sizes, shifts)
    want = E.evaluate(c, five, (LAG, REV), model)
    wl = M.to_limbs(c, want.coefficients)
    keep = [p.coefficients.copy() for p in mirror]
    res = iop.Evaluate(five, None, iop.Form(LAG, REV), *mirror)
    assert (res.Coefficients() == wl).all() and (res.Size(), res.shift) == (want.size, 0) == (1 << 11, 0)
    got, after = run_device(gm, curve, iop.trace(curve, five, 5), mirror, REV)
    assert (got == wl).all()
    for p, k, t in zip(mirror, keep, after):
        assert (p.coefficients == k).all() and (t == k).all()  # inputs unchanged, host and device


# ------------------------------------------------------------------ POINT
@pytest.mark.parametrize("curve", CURVES)
def test_point(gm, curve):
    c, iop = gm.CURVES[curve], gm.iop
    cst = 0xC0FFEE1234567
    f = lambda i, x0, x1: x0 * (cst * i.point()) + x1
    for n in (1, 2, 8, 1 << 11):
        d = gm.fft.NewDomain(curve, n)
        try:
            mirror, model = inputs(gm, curve, n, [REV, REG], tag0=10)
            for out_layout in (REG, REV):
                want = M.to_limbs(c, E.evaluate(c, f, (LAG, out_layout), model, with_point=True).coefficients)
                res = iop.Evaluate(f, None, iop.Form(LAG, out_layout), *mirror, domain=d)
                assert (res.Coefficients() == want).all(), n
            assert (iop.Evaluate(f, None, iop.Form(LAG, REV), *mirror).Coefficients() == want).all()  # the mirror makes the domain
            got, _ = run_device(gm, curve, iop.trace(curve, f, 2), mirror, REV, domain=d)
            assert (got == want).all(), n
            # refused: no domain, a domain of another cardinality
            code = iop.trace(curve, f, 2)
            out = np.zeros((n, c.fr_limbs), dtype=np.uint64)
            with pytest.raises(ValueError, match="POINT needs a domain"):
                iop._expression_call(c, code, None, [p.coefficients.ctypes.data for p in mirror], None, 2, n, [n, n], [0, 0], [REV, REG], REG, 0,
                                     out.ctypes.data_as(ctypes.c_void_p), None)
            other = gm.fft.NewDomain(curve, 2 * n)
            try:
                with pytest.raises(ValueError, match="the domain's cardinality %d is not len %d" % (2 * n, n)):
                    iop.Evaluate(f, out, iop.Form(LAG, REG), *mirror, domain=other)
            finally:
                other.release()
            assert (out == 0).all()
        finally:
            d.release()


# ------------------------------------------------------------------ register pressure
def wide16(i, x):
    squares = [x]
    for _ in range(15):
        squares.append(squares[-1] * squares[-1])  # sixteen values live until the sums
    acc = squares[-1]
    for s in reversed(squares[:-1]):
        acc = acc + s
    return acc


def chain4096(i, x, y):
    acc = x  # INPUT x, INPUT y and 4094 operations: 4096 instructions
    for k in range(4094):
        acc = (acc * x, acc + y, acc - x)[k % 3]
    return acc


@pytest.mark.parametrize("curve", ["bn254", "bw6_761"])
def test_register_pressure(gm, curve):
    c, iop = gm.CURVES[curve], gm.iop
    n = 130  # three workgroups of the 64 lanes a 16-register BW6-761 file leaves, the last ragged
    mirror, model = inputs(gm, curve, n, [REG, REG], tag0=20)
    code = iop.trace(curve, wide16, 1)
    assert E.registers_used(code.words) == 16
    # the model's interpreter, which reduces at every step (the plain callable on exact ints would square 2^15 times unreduced)
    want = M.to_limbs(c, E.run_program(c, code.words, [], model[:1], REG))
    got, _ = run_device(gm, curve, code, mirror[:1], REG)
    assert (got == want).all()
    code = iop.trace(curve, chain4096, 2)
    assert len(code.words) == 4096 and E.registers_used(code.words) <= 3
    want = M.to_limbs(c, E.run_program(c, code.words, [], model, REG))
    got, _ = run_device(gm, curve, code, mirror, REG)
    assert (got == want).all()
    assert (iop.Evaluate(chain4096, None, iop.Form(LAG, REG), *mirror).Coefficients() == want).all()


# ------------------------------------------------------------------ in place
@pytest.mark.parametrize("curve", CURVES)
def test_in_place(gm, curve):
    import torch
    c, iop = gm.CURVES[curve], gm.iop
    n = 1 << 9
    code = iop.trace(curve, E.quotient_expression, 3)
    for layouts, j in (([REG, REV, REG], 2), ([REV, REV, REG], 0)):
        mirror, model = inputs(gm, curve, n, layouts, sizes=[n, n // 2, n], shifts=[0, 3, 0], tag0=30)
        out_layout = layouts[j]
        want = M.to_limbs(c, E.evaluate(c, E.quotient_expression, (COS, out_layout), model).coefficients)
        got, after = run_device(gm, curve, code, mirror, out_layout, out_index=j)
        assert (got == want).all() and (after[j] == want).all()
        for k in range(3):
            if k != j:
                assert (after[k] == mirror[k].coefficients).all()
        host = [p.Clone() for p in mirror]  # the same on host pointers: r is input j's array
        host[j].Shift(0)
        res = iop.Evaluate(E.quotient_expression, host[j].coefficients, iop.Form(COS, out_layout), *host)
        assert res.Coefficients() is host[j].coefficients and (host[j].coefficients == want).all()
    # refused, and nothing written: the other layout, a non-zero offset, a pointer 16 bytes into an input
    mirror, _ = inputs(gm, curve, n, [REG, REV, REG], tag0=30)
    ts = [upload(p.coefficients) for p in mirror]
    torch.cuda.synchronize()
    call = lambda d_out, out_layout, shifts: iop.evaluate_expression_device(curve, code, [t.data_ptr() for t in ts], n, [n] * 3, shifts, [REG, REV, REG],
                                                                            out_layout, d_out)
    same = "the output is input 2, which needs the same layout and no offset"
    with pytest.raises(ValueError, match=same):
        call(ts[2].data_ptr(), REV, [0, 0, 0])
    with pytest.raises(ValueError, match=same):
        call(ts[2].data_ptr(), REG, [0, 0, 1])
    with pytest.raises(ValueError, match="the output overlaps an input"):
        call(ts[2].data_ptr() + 16, REG, [0, 0, 0])
    with pytest.raises(ValueError, match="the output overlaps an input"):
        call(ts[0].data_ptr() - 16, REG, [0, 0, 0])
    for p, t in zip(mirror, ts):
        assert (download(c, t) == p.coefficients).all()


# ------------------------------------------------------------------ the reference's TestDivideByXMinusOne, resident throughout
@pytest.mark.parametrize("n", [8, 1 << 9])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_pipeline_resident(gm, curve, n):
    import torch
    c, iop = gm.CURVES[curve], gm.iop
    r, N = c.r, 4 * n
    _, va = vector(gm, curve, 40, n)
    _, vb = vector(gm, curve, 41, n)
    vc = [(x * x * x - x * x * y) % r for x, y in zip(va, vb)]  # the instance on which h vanishes over the small domain
    mdom = (P.Domain(c, n), P.Domain(c, N))
    # the model: canonical coefficients, the big coset, the numerator, the quotient
    mcan = [P.to_regular(P.to_canonical(P.Polynomial(v, LAG, REG), mdom[0])) for v in (va, vb, vc)]
    mcos = []
    for p in mcan:
        q = p.clone()
        q.size = n
        mcos.append(P.to_lagrange_coset(q, mdom[1]))  # Canonical Regular -> LagrangeCoset BitReverse, grown to N
    mnum = E.evaluate(c, E.quotient_expression, (COS, REV), mcos)
    mnum.size = n
    mquot = P.divide_by_x_minus_one(mnum, mdom)
    doms = (gm.fft.NewDomain(curve, n), gm.fft.NewDomain(curve, N))
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ts = []
            for p in mcan:
                buf = np.full((N, c.fr_limbs), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)  # the tail is garbage until the entry grows it
                buf[:n] = M.to_limbs(c, p.coefficients)
                t = upload(buf)
                assert iop.to_basis_device(doms[1], t.data_ptr(), n, iop.Form(CAN, REG), COS, s.cuda_stream) == REV
                ts.append(t)
            num, quot = upload(np.zeros((N, c.fr_limbs), dtype=np.uint64)), upload(np.zeros((N, c.fr_limbs), dtype=np.uint64))
            iop.evaluate_expression_device(curve, iop.trace(curve, E.quotient_expression, 3), [t.data_ptr() for t in ts], N, [n] * 3, [0] * 3,
                                           [REV] * 3, REV, num.data_ptr(), stream=s.cuda_stream)
            iop.divide_by_x_minus_one_device(doms, num.data_ptr(), iop.Form(COS, REV), 0, quot.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert (download(c, num) == M.to_limbs(c, mnum.coefficients)).all()
        assert (mquot.basis, mquot.layout) == (CAN, REG)
        assert (download(c, quot) == M.to_limbs(c, mquot.coefficients)).all()
        assert mquot.coefficients[2 * n:] == [0] * (2 * n) and any(mquot.coefficients)  # degree 3(n - 1) - n: h vanishes on the small domain
    finally:
        for d in doms:
            d.release()


# ------------------------------------------------------------------ threads
@pytest.mark.parametrize("curve", CURVES)
def test_four_threads_each_with_its_own_program(gm, curve):
    import torch
    c, iop = gm.CURVES[curve], gm.iop
    n = 1 << 10
    fs = [E.quotient_expression, lambda i, a, b, c_: a * b - c_, lambda i, a, b, c_: -(a + b) * (c_ + 7), lambda i, a, b, c_: a * i.point() + b * c_]
    jobs = [([REG, REV, REG], REG), ([REV, REV, REV], REV), ([REG, REG, REG], REV), ([REV, REG, REV], REG)]
    d = gm.fft.NewDomain(curve, n)
    try:
        cases = []
        for f, (layouts, out_layout) in zip(fs, jobs):
            mirror, model = inputs(gm, curve, n, layouts, tag0=50)
            code = iop.trace(curve, f, 3)
            want = M.to_limbs(c, E.evaluate(c, f, (LAG, out_layout), model, with_point=code.has_point).coefficients)
            cases.append((code, mirror, out_layout, want))
        errs = []

        def run(k):
            try:
                code, mirror, out_layout, want = cases[k]
                for _ in range(3):
                    got, _ = run_device(gm, curve, code, mirror, out_layout, domain=d if code.has_point else None)
                    assert (got == want).all()
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=run, args=(k,)) for k in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        torch.cuda.synchronize()
    finally:
        d.release()


# ------------------------------------------------------------------ profiling
def test_profiling_goes_to_stage_slot_0(gm):
    lib, iop = gm._lib.load(), gm.iop
    mirror, _ = inputs(gm, "bn254", 1 << 11, [REG, REV, REG])
    lib.gmsm_set_profiling(1)  # resets the accumulators
    try:
        for _ in range(3):
            iop.Evaluate(E.quotient_expression, None, iop.Form(COS, REG), *mirror)
        ms, calls = (ctypes.c_double * 8)(), ctypes.c_ulong(0)
        assert lib.gmsm_get_stage_times(ms, 8, ctypes.byref(calls)) == 8
    finally:
        lib.gmsm_set_profiling(0)
    assert calls.value == 3 and ms[0] > 0
