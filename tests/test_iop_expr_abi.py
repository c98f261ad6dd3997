"""gmsm_iop_evaluate_expression of include/gmsm.h without a device: the symbol is exported, declared with the stated arity and
bound; the opcode constants and limits of the header are those of the mirror (gnark-crypto_amd/iop.py); every error the host
can decide - of the program (each names the instruction index) and of the call - returns GMSM_ERR_ARG with its text before any
device work, and nothing is written; the mirror raises the reference's texts. And what can be checked of
integration/go/<curve>/iop/expressions_*.go without a Go toolchain, as tests/test_iop_poly_abi.py does for its files: build
tags, package, the same exported signatures in both builds, the C call declared and exported with the prototype's arity, the
three curve directories equal up to the documented substitutions."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
SYM, ARITY = "gmsm_iop_evaluate_expression", 17
CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
EXPORTED = ["NewProgram", "Input", "Const", "Point", "Add", "Sub", "Mul", "Neg", "EvaluateDevice"]
ARG = 4  # GMSM_ERR_ARG
INPUT, CONST, POINT, ADD, SUB, MUL, NEG = 1, 2, 3, 4, 5, 6, 7


def header():
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        return f.read()


def test_symbol_is_exported_declared_and_bound(gm):
    lib = gm._lib.load()
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert SYM in gm._lib.ABI_SYMBOLS
    f = getattr(lib, SYM)
    assert f.restype is ctypes.c_int
    proto = re.search(rf"^int {SYM}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
    assert proto
    assert len(f.argtypes) == proto.group(1).count(",") + 1 == ARITY


def test_header_constants_are_the_mirrors(gm):
    h = header()
    defs = {name: int(v) for name, v in re.findall(r"^#define GMSM_EXPR_([A-Z_]+) (\d+)$", h, re.M)}
    iop = gm.iop
    assert defs == {"INPUT": iop.EXPR_INPUT, "CONST": iop.EXPR_CONST, "POINT": iop.EXPR_POINT, "ADD": iop.EXPR_ADD, "SUB": iop.EXPR_SUB,
                    "MUL": iop.EXPR_MUL, "NEG": iop.EXPR_NEG, "MAX_REGS": iop.EXPR_MAX_REGS, "MAX_INSNS": iop.EXPR_MAX_INSNS,
                    "MAX_INPUTS": iop.EXPR_MAX_INPUTS, "MAX_CONSTS": iop.EXPR_MAX_CONSTS}
    assert (defs["MAX_REGS"], defs["MAX_INSNS"], defs["MAX_INPUTS"], defs["MAX_CONSTS"]) == (16, 4096, 64, 256)
    assert sorted(defs[k] for k in ("INPUT", "CONST", "POINT", "ADD", "SUB", "MUL", "NEG")) == list(range(1, 8))
    doc = re.sub(r"\s*\n \*\s*", " ", h[h.index("iop.Evaluate (ecc"):h.index("#define GMSM_EXPR_INPUT")])
    for text in ("op | dst << 8 | a << 16 | b << 24", "The value of the expression is the dst of the last instruction",
                 "the inputs are NOT concatenated", "the lane that reads a slot is then the one that writes it",
                 "len == 0 is GMSM_OK and touches nothing", "names the instruction index"):
        assert text in doc, text


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ins(op, dst=0, a=0, b=0):
    return op | dst << 8 | a << 16 | b << 24


def test_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    E = SYM + ": "
    n = 8
    a, b, out = (np.zeros((n, 4), dtype=np.uint64) for _ in range(3))
    a[:], b[:] = 3, 5
    consts = np.zeros((2, 4), dtype=np.uint64)
    nohandle = 1 << 40
    good = [ins(INPUT, 0, 0), ins(INPUT, 1, 1), ins(MUL, 0, 0, 1)]

    def call(prog=good, group=0, domain=0, n_consts=2, polys=(a, b), d_polys=None, m=None, length=n, sizes=None, shifts=None, layouts=None,
             out_layout=8, o=out, d_out=None, prog_len=None, null=()):
        words = np.array(prog if len(prog) else [0], dtype=np.uint32)
        m = (len(polys) if polys is not None else len(d_polys)) if m is None else m
        k = max(m, 1)
        arr = lambda src: None if src is None else (ctypes.c_void_p * max(len(src), 1))(*[x if isinstance(x, int) else x.ctypes.data for x in src])
        sz = np.array(sizes if sizes is not None else [length] * k, dtype=np.uintp)
        sh = np.array(shifts if shifts is not None else [0] * k, dtype=np.int64)
        lay = np.array(layouts if layouts is not None else [8] * k, dtype=np.uint32)
        keep = (arr(polys), arr(d_polys))
        return lib.gmsm_iop_evaluate_expression(
            group, domain, None if "prog" in null else words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(prog) if prog_len is None else prog_len,
            None if "consts" in null else _p(consts), n_consts, keep[0], keep[1], m, length,
            None if "sizes" in null else sz.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
            None if "shifts" in null else sh.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            None if "layouts" in null else lay.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out_layout, None, None if o is None else _p(o), d_out)

    assert call(group=99) == ARG and "unknown group" in err()
    assert call(length=0) == 0  # GMSM_OK, nothing touched, whatever else is wrong
    assert call(length=0, prog=[], m=0, polys=None) == 0
    # ---- the program (§1): each text names the instruction index
    assert call(prog=[]) == ARG and err() == E + "empty program"
    assert call(prog=good, prog_len=4097) == ARG and err() == E + "the program has 4097 instructions, more than 4096"
    assert call(prog=good + [ins(9, 2, 0, 1)]) == ARG and err() == E + "instruction 3: unknown opcode 9"
    assert call(prog=[ins(0)]) == ARG and err() == E + "instruction 0: unknown opcode 0"
    assert call(prog=[ins(INPUT, 16, 0)]) == ARG and err() == E + "instruction 0: register 16 is not below 16"
    assert call(prog=good + [ins(ADD, 0, 17, 0)]) == ARG and err() == E + "instruction 3: register 17 is not below 16"
    assert call(prog=good + [ins(ADD, 0, 0, 255)]) == ARG and err() == E + "instruction 3: register 255 is not below 16"
    assert call(prog=[ins(INPUT, 0, 0), ins(ADD, 1, 0, 1)]) == ARG and err() == E + "instruction 1: reads register 1 before any instruction wrote it"
    assert call(prog=[ins(NEG, 0, 0)]) == ARG and err() == E + "instruction 0: reads register 0 before any instruction wrote it"
    assert call(prog=good + [ins(INPUT, 2, 2)]) == ARG and err() == E + "instruction 3: input 2 of 2"
    assert call(prog=good + [ins(CONST, 2, 2)]) == ARG and err() == E + "instruction 3: constant 2 of 2"
    assert call(prog=[ins(CONST, 0, 0)], n_consts=0, null=("consts",)) == ARG and err() == E + "instruction 0: constant 0 of 0"
    assert call(prog=good + [ins(POINT, 2)]) == ARG and err() == E + "instruction 3: POINT needs a domain (domain == 0)"
    # ---- the call (§2)
    assert call(m=0, polys=()) == ARG and err() == E + "need at least one input (m == 0)"
    assert call(m=65) == ARG and err() == E + "65 inputs, more than 64"
    assert call(n_consts=257) == ARG and err() == E + "257 constants, more than 256"
    assert call(null=("prog",)) == ARG and err() == E + "prog is null"
    assert call(null=("consts",)) == ARG and err() == E + "consts is null"
    assert call(null=("sizes",)) == ARG and call(null=("shifts",)) == ARG and err() == E + "sizes and shifts must not be null"
    assert call(null=("layouts",)) == ARG and err() == E + "layouts is null"
    assert call(layouts=[8, 4]) == ARG and err() == E + "layouts[1] = 4 is no layout (8 Regular, 16 BitReverse)"
    assert call(out_layout=0) == ARG and err() == E + "unknown layout 0 (8 Regular, 16 BitReverse)"
    one_of = lambda h, d: E + f"give exactly one of {h} (host) / {d} (device)"
    assert call(polys=None, m=2) == ARG and err() == one_of("polys", "d_polys")  # d_polys None as well
    assert call(d_polys=(a, b)) == ARG and err() == one_of("polys", "d_polys")
    assert call(o=None) == ARG and err() == one_of("out", "d_out")
    assert call(d_out=_p(out)) == ARG and err() == one_of("out", "d_out")
    assert call(polys=(a, 0)) == ARG and err() == E + "polys[1] is null"
    assert call(sizes=[n, 0]) == ARG and err() == E + "sizes[1] = 0 is outside [1, len]"
    assert call(sizes=[n + 1, n]) == ARG and err() == E + "sizes[0] = 9 is outside [1, len]"
    assert call(shifts=[0, -1]) == ARG and err() == E + "shifts[1] = -1 is negative (the reference panics on the index)"
    pow2 = E + "len must be a power of 2 with a BitReverse layout or a POINT instruction"
    assert call(length=6, layouts=[8, 16]) == ARG and err() == pow2
    assert call(length=6, out_layout=16) == ARG and err() == pow2
    assert call(length=6, prog=good + [ins(POINT, 2)], domain=nohandle) == ARG and err() == pow2
    assert call(domain=nohandle) == ARG and err() == "unknown fft domain handle"
    assert call(prog=good + [ins(POINT, 2)], domain=nohandle) == ARG and err() == "unknown fft domain handle"
    # ---- the output and the inputs: in place needs the same layout and no offset; any other shared byte is refused
    overlaps = "the output overlaps an input (inputs are never modified)"
    big = np.zeros((2 * n, 4), dtype=np.uint64)
    assert call(polys=(big[:n], b), o=big[1:n + 1]) == ARG and err().endswith(overlaps)
    assert call(polys=(a, big[n // 2:]), o=big[:n]) == ARG and err().endswith(overlaps)
    same = E + "the output is input 1, which needs the same layout and no offset (the lane that reads a slot must be the one that writes it)"
    assert call(o=b, layouts=[8, 16]) == ARG and err() == same
    assert call(o=b, out_layout=16) == ARG and err() == same
    assert call(o=b, shifts=[0, 3]) == ARG and err() == same
    assert call(o=b, sizes=[n, n // 2], shifts=[0, 1]) == ARG and err() == same  # offset rho shift = 2
    assert call(o=a, polys=(a, a), layouts=[8, 16]) == ARG and err().startswith(E + "the output is input 1")
    assert (out == 0).all() and (a == 3).all() and (b == 5).all() and (big == 0).all()


def test_mirror_raises_the_reference_errors(gm):
    iop = gm.iop
    c = gm.CURVES["bn254"]
    form = iop.Form(iop.Lagrange, iop.Regular)
    z8, z4 = np.zeros((8, c.fr_limbs), dtype=np.uint64), np.zeros((4, c.fr_limbs), dtype=np.uint64)
    p8, p4 = iop.NewPolynomial("bn254", z8, form), iop.NewPolynomial("bn254", z4, form)
    f = lambda i, x, y: x * y
    with pytest.raises(ValueError) as e:
        iop.Evaluate(f, None, form)
    assert str(e.value) == "need at lest one input"  # the reference's text (expressions.go:39)
    with pytest.raises(ValueError) as e:
        iop.Evaluate(f, None, form, p8, p4)
    assert str(e.value) == iop.ErrInconsistentSize
    with pytest.raises(ValueError) as e:
        iop.Evaluate(f, z4, form, p8, p8)
    assert str(e.value) == iop.ErrInconsistentSize
    with pytest.raises(ValueError, match="more than 16 registers are live"):
        iop.Evaluate(lambda i, x: _wide(x), None, form, p8)
    with pytest.raises(ValueError, match=r"shifts\[0\] = -2 is negative"):
        iop.Evaluate(lambda i, x: x + x, None, form, iop.NewPolynomial("bn254", z8, form).Shift(-2))
    with pytest.raises(ValueError, match="the output is input 0, which needs the same layout and no offset"):
        iop.Evaluate(lambda i, x: x + x, z8, iop.Form(iop.Lagrange, iop.BitReverse), p8)
    assert callable(iop.evaluate_expression_device) and callable(iop.trace) and callable(iop.Program)


def _wide(x):
    squares = [x]
    for _ in range(16):
        squares.append(squares[-1] * squares[-1])
    acc = squares[-1]
    for s in reversed(squares[:-1]):
        acc = acc + s
    return acc


# ---- the Go files
def read(curve, name):
    with open(os.path.join(GO, curve, "iop", name)) as f:
        return f.read()


def call_arities(text, sym):
    out = []
    for m in re.finditer(rf"C\.{sym}\(", text):
        depth, i, commas = 1, m.end(), 0
        while depth:
            ch = text[i]
            depth += ch == "("
            depth -= ch == ")"
            commas += (ch == "," and depth == 1)
            i += 1
        out.append(0 if not text[m.end():i - 1].strip() else commas + 1)
    return out


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_go_files(gm, curve):
    path, ids = CURVES[curve]
    dev, pure = read(curve, "expressions_mi355x.go"), read(curve, "expressions_purego.go")
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    exported = lambda text: re.findall(r"^func (?:\(\w+ \*Program\) )?([A-Z]\w*)\(", text, re.M)
    for text in (dev, pure):
        assert re.search(r"^package iop$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and f'"github.com/consensys/gnark-crypto/{path}/fr/fft"' in text
        assert exported(text) == EXPORTED  # the same exported functions and methods in both builds
        assert re.search(r"^type Program struct \{$", text, re.M) and re.search(r"^type Sym int$", text, re.M)
        opcodes = re.search(r"const \(\n\texprInput = 1 \+ iota\n\texprConst\n\texprPoint\n\texprAdd\n\texprSub\n\texprMul\n\texprNeg\n\texprMaxRegs = 16\n\)", text)
        assert opcodes  # 1..7 in the header's order
    sig = lambda text: re.findall(r"^func ((?:\(\w+ \*Program\) )?[A-Z]\w*\(.*)\{$", text, re.M)
    assert sig(dev) == sig(pure) and len(sig(dev)) == len(EXPORTED)  # ... with the same signatures
    assert "func EvaluateDevice(p *Program, r []fr.Element, form Form, x ...*Polynomial) (*Polynomial, error) {" in dev
    assert 'import "C"' not in pure and "C." not in re.sub(r"//.*", "", pure)
    assert "return Evaluate(f, r, form, x...)" in pure  # the build without the tag goes through the reference's Evaluate
    for ref in ("ErrInconsistentSize", '"need at lest one input"', "gmsmDomain(", "runtime.Pinner", "res.size = x[0].size"):
        assert ref in dev  # the reference's checks and result stay in the wrapper; the pointer array is pinned
    assert "func gmsmDomain(" not in dev and "func gmsmElems(" not in dev  # they come from ratios_mi355x.go
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert called == {SYM}
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = gm._lib.load()
    assert hasattr(lib, SYM)
    proto = re.search(rf"\b{SYM}\s*\(([^;]*?)\)\s*;", decls, re.S)
    assert set(call_arities(dev, SYM)) == {proto.group(1).count(",") + 1} == {ARITY}


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, ids = CURVES[curve]
    for name in ("expressions_mi355x.go", "expressions_purego.go"):
        base = read("bn254", name).replace("ecc/bn254", path).replace("GMSM_BN254_", ids)
        assert base == read(curve, name), name
