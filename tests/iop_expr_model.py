"""Python big-int model of iop.Evaluate (ecc/<curve>/fr/iop/expressions.go:26-73) and of the straight-line programs that
gmsm_iop_evaluate_expression interprets (include/gmsm.h, GMSM_EXPR_*), shared by tests/test_iop_expr_model.py (no GPU, no
library) and tests/test_gpu_iop_expr.py.

Everything works on TRUE values mod r (plain Python ints; iop_model.from_limbs / to_limbs convert the Montgomery limbs the C
ABI speaks). Two parts:
  - evaluate: the reference's loop, literally - GetCoeff with rho and shift per input, the index map of the result's layout -
    over a plain Python callable f(i, *x). x are ints and + - * on them are exact, so reducing f's value once mod r is the
    field's result; i is an Index whose point() is w^i (the only use the device form allows of i)
  - run_program: an interpreter of the instruction words, register by register"""
import iop_model as M
import iop_poly_model as P

REGULAR, BIT_REVERSE = M.REGULAR, M.BIT_REVERSE
INPUT, CONST, POINT, ADD, SUB, MUL, NEG = 1, 2, 3, 4, 5, 6, 7
MAX_REGS = 16


class Index(int):
    """the closure's argument i: an int that also knows w^i"""

    def __new__(cls, i, w, r):
        self = super().__new__(cls, i)
        self.w, self.r = w, r
        return self

    def point(self):
        return pow(self.w, int(self), self.r)


def _omega(curve, n, with_point):
    return M.generator(curve, n) if with_point else None


def evaluate(curve, f, form, polys, with_point=False):
    """Evaluate(f, nil, form, polys...) (expressions.go:37-73): polys are iop_poly_model.Polynomial; the result's coefficients
    in form's layout, size of polys[0], shift 0"""
    n = len(polys[0].coefficients)
    assert all(len(p.coefficients) == n for p in polys)  # ErrInconsistentSize
    r, w = curve.r, _omega(curve, n, with_point)
    out = [0] * n
    for i in range(n):
        vx = [P.get_coeff(p, i) for p in polys]
        out[i if form[1] == REGULAR else M.bit_reverse_index(i, n)] = f(Index(i, w, r), *vx) % r
    res = P.Polynomial(out, form[0], form[1])
    res.size = polys[0].size
    return res


def run_program(curve, words, consts, polys, out_layout, with_point=False):
    """the program at every index: words are op | dst << 8 | a << 16 | b << 24, consts true values, polys
    iop_poly_model.Polynomial (their size and shift enter through GetCoeff); asserts what the C entry validates"""
    n = len(polys[0].coefficients)
    r, w = curve.r, _omega(curve, n, with_point)
    assert 0 < len(words) <= 4096
    out = [0] * n
    for i in range(n):
        reg, last = {}, None
        for ins in words:
            ins = int(ins)
            op, dst, a, b = ins & 0xFF, (ins >> 8) & 0xFF, (ins >> 16) & 0xFF, ins >> 24
            assert dst < MAX_REGS
            if op == INPUT:
                v = P.get_coeff(polys[a], i)
            elif op == CONST:
                v = consts[a] % r
            elif op == POINT:
                assert w is not None, "POINT without a domain"
                v = pow(w, i, r)
            elif op == ADD:
                v = (reg[a] + reg[b]) % r
            elif op == SUB:
                v = (reg[a] - reg[b]) % r
            elif op == MUL:
                v = reg[a] * reg[b] % r
            elif op == NEG:
                v = -reg[a] % r
            else:
                raise AssertionError("unknown opcode %d" % op)
            reg[dst] = last = v
        out[i if out_layout == REGULAR else M.bit_reverse_index(i, n)] = last
    return out


def registers_used(words):
    return len({(int(w) >> 8) & 0xFF for w in words})


# the expressions of the reference's own tests and of the timing tool
def sum_expression(i, x0, x1, x2):  # expressions_test.go:16-20
    return x0 + x1 + x2


def quotient_expression(i, x0, x1, x2):  # quotient_test.go:35-41: h = x1^2 x2 + x3 - x1^3
    return x0 * x0 * x1 + x2 - x0 * x0 * x0


def random_tree(rng, depth, m, with_point):
    """a random expression over m inputs as a callable f(i, *x): nested tuples of + - * neg, leaves inputs, small and
    full-size constants and, when asked, i.point(); depth <= 6. Returns (f, uses_point)."""
    used = [False]

    def make(d):
        k = int(rng.integers(0, 10))
        if d == 0 or k == 0:
            leaf = int(rng.integers(0, 4 if with_point else 3))
            if leaf == 0 or leaf == 1:
                return ("x", int(rng.integers(0, m)))
            if leaf == 2:
                return ("c", int(rng.integers(0, 1 << 62)) ** int(rng.integers(1, 5)) - int(rng.integers(0, 3)))
            used[0] = True
            return ("w",)
        if k == 1:
            return ("neg", make(d - 1))
        return (("add", "sub", "mul")[k % 3], make(d - 1), make(d - 1))

    tree = make(depth)

    def run(t, i, x):
        if t[0] == "x":
            return x[t[1]]
        if t[0] == "c":
            return t[1]  # a plain int: the symbols turn it into a constant, the ints take it as it is
        if t[0] == "w":
            return i.point()
        if t[0] == "neg":
            return -run(t[1], i, x)
        a, b = run(t[1], i, x), run(t[2], i, x)
        return a + b if t[0] == "add" else a - b if t[0] == "sub" else a * b

    return (lambda i, *x: run(tree, i, x)), used[0]
