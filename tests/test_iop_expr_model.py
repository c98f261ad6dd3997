"""Pins the tracer of gnark-crypto_amd/iop.py (Program, trace) and tests/iop_expr_model.py (the big-int model the GPU tests
compare against) to each other without a GPU or the library:
  - the traced program, run by the model's interpreter, equals the reference's loop over the plain callable on random
    expression trees (depth <= 6, up to 5 inputs, constants, point()) for the three scalar fields, with sizes, shifts and
    mixed layouts on the inputs and both layouts of the result
  - registers are allocated by liveness: a chain of 40 products needs at most 3, a symbol used twice is computed once, a
    17-wide live set raises, constants that the result does not need do not travel
  - the reference's TestEvaluate on the model: u[i] = i, v = u + 1, w = u + 2, layouts switched to BitReverse one after
    another; the Regular-layout result is 3 (i + 1) all three times"""
import numpy as np
import pytest

import iop_expr_model as E
import iop_model as M
import iop_poly_model as P
from conftest import rng_for

CURVES = ["bn254", "bls12_381", "bw6_761"]


def code_of(gm, curve, f, m):
    code = gm.iop.trace(curve, f, m)
    return code.words, M.from_limbs(gm.CURVES[curve], code.consts), code.has_point


@pytest.mark.parametrize("curve", CURVES)
def test_traced_program_equals_the_plain_callable_on_random_trees(gm, curve):
    c = gm.CURVES[curve]
    rng = rng_for(0xE8, CURVES.index(curve))
    n = 8
    pointed = 0
    for case in range(24):
        m = 1 + case % 5
        f, uses_point = E.random_tree(rng, 1 + case % 6, m, with_point=case % 2 == 1)
        pointed += uses_point
        polys = []
        for j in range(m):
            p = P.Polynomial([int(rng.integers(0, 1 << 63)) ** 5 % c.r for _ in range(n)], P.LAGRANGE, (E.REGULAR, E.BIT_REVERSE)[(case + j) % 2])
            p.size, p.shift = (8, 4, 2)[j % 3], (0, 1, 3)[(case + j) % 3]
            polys.append(p)
        words, consts, has_point = code_of(gm, curve, f, m)
        assert has_point == uses_point
        # a tree of depth 6 evaluated left to right holds at most 7 values; an input or the point that is used again later
        # keeps its register meanwhile: 5 + 1 more
        assert E.registers_used(words) <= 13 and len(words) < 1 << 8
        for layout in (E.REGULAR, E.BIT_REVERSE):
            want = E.evaluate(c, f, (P.LAGRANGE, layout), polys, with_point=uses_point)
            assert E.run_program(c, words, consts, polys, layout, with_point=uses_point) == want.coefficients, case
            assert (want.size, want.shift) == (polys[0].size, 0)
    assert pointed >= 4


def test_registers_are_reused(gm):
    iop = gm.iop

    def chain(i, x):
        acc = x
        for _ in range(40):
            acc = acc * x
        return acc
    code = iop.trace("bn254", chain, 1)
    assert len(code.words) == 41 and E.registers_used(code.words) <= 3
    c = gm.CURVES["bn254"]
    p = P.Polynomial([3, 5], P.CANONICAL, E.REGULAR)
    assert E.run_program(c, code.words, [], [p], E.REGULAR) == [pow(3, 41, c.r), pow(5, 41, c.r)]

    # a symbol used twice is computed once; what the result does not need is not emitted
    def shared(i, a, b):
        s = a + b
        unused = a * 12345  # noqa: F841
        return s * s - s
    code = iop.trace("bn254", shared, 2)
    ops = [int(w) & 0xFF for w in code.words]
    assert ops == [E.INPUT, E.INPUT, E.ADD, E.MUL, E.SUB] and code.consts.shape == (0, c.fr_limbs) and not code.has_point
    # the inputs of a traced function are loaded where they are first used, not all at the start
    code = iop.trace("bn254", lambda i, *x: sum(x[1:], x[0]), 40)
    assert E.registers_used(code.words) == 2 and len(code.words) == 79


def test_a_17_wide_live_set_raises(gm):
    iop = gm.iop

    def wide(k):
        def f(i, x):
            squares = [x]
            for _ in range(k - 1):
                squares.append(squares[-1] * squares[-1])  # all of them stay live until the sums below
            acc = squares[-1]
            for s in reversed(squares[:-1]):
                acc = acc + s
            return acc
        return f
    code = iop.trace("bw6_761", wide(16), 1)
    assert E.registers_used(code.words) == 16
    with pytest.raises(ValueError, match="more than 16 registers are live"):
        iop.trace("bw6_761", wide(17), 1)
    p = iop.Program("bn254")
    with pytest.raises(ValueError, match="symbols of two programs"):
        p.input(0) + iop.Program("bn254").input(0)


def test_builder_methods_and_constants(gm):
    iop = gm.iop
    c = gm.CURVES["bls12_381"]
    p = iop.Program("bls12_381")
    x, w = p.input(0), p.point()
    five = p.const(5)
    assert p.const(5 + c.r) is five and p.input(0) is x and p.point() is w and p.index().point() is w
    limbs = M.to_limbs(c, [7])[0]
    code = p.build(-(x * five) + w * limbs + 2 - x)
    assert code.has_point and code.words.dtype == np.uint32 and code.consts.dtype == np.uint64
    assert M.from_limbs(c, code.consts) == [5, 7, 2]
    poly = P.Polynomial([11, 13, 17, 19], P.LAGRANGE, E.REGULAR)
    wgen = M.generator(c, 4)
    want = [(-(v * 5) + pow(wgen, i, c.r) * 7 + 2 - v) % c.r for i, v in enumerate(poly.coefficients)]
    assert E.run_program(c, code.words, [5, 7, 2], [poly], E.REGULAR, with_point=True) == want
    # a result that is no symbol is a constant; a leaf alone is a program of one instruction
    assert [int(v) & 0xFF for v in iop.trace("bn254", lambda i, a: 9, 1).words] == [E.CONST]
    assert [int(v) for v in iop.trace("bn254", lambda i, a, b: b, 2).words] == [E.INPUT | 0 << 8 | 1 << 16]
    assert (iop.EXPR_INPUT, iop.EXPR_CONST, iop.EXPR_POINT, iop.EXPR_ADD, iop.EXPR_SUB, iop.EXPR_MUL, iop.EXPR_NEG) == (
        E.INPUT, E.CONST, E.POINT, E.ADD, E.SUB, E.MUL, E.NEG)


@pytest.mark.parametrize("curve", CURVES)
def test_reference_test_evaluate_on_the_model(gm, curve):
    c = gm.CURVES[curve]
    size = 64
    polys = [P.Polynomial([i + k for i in range(size)], P.CANONICAL, E.REGULAR) for k in range(3)]
    words, consts, _ = code_of(gm, curve, E.sum_expression, 3)
    expected = [3 * (i + 1) for i in range(size)]
    form = (P.CANONICAL, E.REGULAR)
    for step in range(3):  # all Regular; u BitReverse; u, v, w BitReverse
        if step == 1:
            P.to_bit_reverse(polys[0])
        if step == 2:
            P.to_bit_reverse(polys[1]), P.to_bit_reverse(polys[2])
        assert E.evaluate(c, E.sum_expression, form, polys).coefficients == expected
        assert E.run_program(c, words, consts, polys, E.REGULAR) == expected
    assert [p.layout for p in polys] == [E.BIT_REVERSE] * 3
