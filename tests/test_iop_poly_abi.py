"""The iop.Polynomial entries of include/gmsm.h without a device: the three symbols are exported, declared with the stated
arity and bound; every argument error the host can decide returns GMSM_ERR_ARG with its text before any device work; the
header states the three departures from the reference; the mirror (gnark-crypto_amd/iop.py) raises the reference's texts.
And what can be checked of integration/go/<curve>/iop/polynomial_*.go without a Go toolchain, as tests/test_iop_abi.py does
for the ratio files: build tags, package, the same exported signatures in both builds, C calls declared and exported with the
prototypes' arity, the three curve directories equal up to the documented substitutions."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
SYMBOLS = {"gmsm_iop_to_basis": 9, "gmsm_iop_evaluate": 13, "gmsm_iop_divide_by_x_minus_one": 10}
CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
EXPORTED = ["ToLagrangeDevice", "ToCanonicalDevice", "ToLagrangeCosetDevice", "EvaluateDevice", "DivideByXMinusOneDevice"]
ARG = 4  # GMSM_ERR_ARG
U32P = ctypes.POINTER(ctypes.c_uint32)


def header():
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        return f.read()


def test_symbols_are_exported_declared_and_bound(gm):
    lib = gm._lib.load()
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for sym, arity in SYMBOLS.items():
        assert sym in gm._lib.ABI_SYMBOLS
        f = getattr(lib, sym)
        assert f.restype is ctypes.c_int
        proto = re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
        assert proto, sym
        assert len(f.argtypes) == proto.group(1).count(",") + 1 == arity, sym


def test_header_states_the_departures():
    h = header()
    doc = re.sub(r"\s*\n \*\s*", " ", h[h.index("iop.Polynomial (ecc"):h.index("int gmsm_iop_to_basis(")])
    assert "the result is 0: the reference's answer, NOT the interpolated value" in doc  # x on the domain
    assert "a shift outside 0..5 is refused" in doc and "that defect is not reproduced" in doc
    assert "has coset 0 and is evaluated at 0" in doc and "0^-1 = 0" in doc
    assert "the basis must be LagrangeCoset" in doc and "IN PLACE" in doc and "the reference's grow" in doc


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    a, out = np.zeros((8, 4), dtype=np.uint64), np.zeros((8, 4), dtype=np.uint64)
    x = np.zeros(4, dtype=np.uint64)
    lay_out = ctypes.c_int(0)
    nohandle = 1 << 40
    one_of = lambda h, d: f"give exactly one of {h} (host) / {d} (device)"

    tb = lib.gmsm_iop_to_basis
    TB = "gmsm_iop_to_basis: "
    for h, d in ((None, None), (_p(a), _p(a))):
        assert tb(nohandle, h, d, 8, 1, 8, 2, None, ctypes.byref(lay_out)) == ARG and err() == TB + one_of("a", "d_a")
    for basis in (0, 3, 8):
        assert tb(nohandle, _p(a), None, 8, basis, 8, 2, None, ctypes.byref(lay_out)) == ARG and TB + f"unknown basis {basis}" in err()
        assert tb(nohandle, _p(a), None, 8, 2, 8, basis, None, ctypes.byref(lay_out)) == ARG and TB + f"unknown to_basis {basis}" in err()
    for layout in (0, 1, 24):
        assert tb(nohandle, _p(a), None, 8, 1, layout, 2, None, ctypes.byref(lay_out)) == ARG and TB + f"unknown layout {layout}" in err()
    assert tb(nohandle, _p(a), None, 8, 1, 8, 2, None, None) == ARG and err() == TB + "out_layout is null"
    assert tb(nohandle, _p(a), None, 8, 1, 8, 2, None, ctypes.byref(lay_out)) == ARG and err() == "unknown fft domain handle"
    assert tb(0, _p(a), None, 8, 4, 16, 4, None, ctypes.byref(lay_out)) == ARG and err() == "unknown fft domain handle"
    assert (a == 0).all()

    ev = lib.gmsm_iop_evaluate
    EV = "gmsm_iop_evaluate: "
    lp = lambda v: np.array(v, dtype=np.uint32).ctypes.data_as(U32P)
    reg, rev, mixed = lp([8, 8]), lp([16, 16]), lp([8, 16])
    call = lambda group=0, polys=_p(a), d_polys=None, k=2, n=4, size=4, basis=2, lay=reg, shift=0, coset=_p(x), xx=_p(x), o=_p(out): ev(
        group, polys, d_polys, k, n, size, basis, lay, shift, coset, xx, None, o)
    assert call(group=99) == ARG and "unknown group" in err()
    assert call(k=0) == ARG and err() == EV + "no polynomial (k == 0)"
    assert call(n=0) == ARG and err() == EV + "empty polynomial (len == 0)"
    assert call(size=0) == ARG and err() == EV + "size == 0"
    for basis in (0, 3, 16):
        assert call(basis=basis) == ARG and EV + f"unknown basis {basis}" in err()
    assert call(lay=None) == ARG and err() == EV + "layouts is null"
    assert call(lay=lp([8, 4])) == ARG and err() == EV + "layouts[1] = 4 is no layout (8 Regular, 16 BitReverse)"
    assert call(lay=lp([0, 16])) == ARG and err() == EV + "layouts[0] = 0 is no layout (8 Regular, 16 BitReverse)"
    assert call(polys=None) == ARG and err() == EV + one_of("polys", "d_polys")
    assert call(d_polys=_p(a)) == ARG and err() == EV + one_of("polys", "d_polys")
    assert call(xx=None) == ARG and err() == EV + "x and out_values must not be null"
    assert call(o=None) == ARG and err() == EV + "x and out_values must not be null"
    assert call(basis=4, coset=None) == ARG and err() == EV + "coset is null and the basis is LagrangeCoset"
    for shift in (6, 7, 1 << 20):
        assert call(basis=1, shift=shift) == ARG and EV + f"shift {shift} is outside 0..5" in err()
    pow2 = EV + "len must be a power of 2 in a Lagrange basis or a BitReverse layout"
    assert call(k=1, n=6, basis=2) == ARG and err() == pow2
    assert call(k=1, n=6, basis=4) == ARG and err() == pow2
    assert call(k=1, n=3, basis=1, lay=rev) == ARG and err() == pow2
    assert call(k=2, n=3, basis=1, lay=mixed) == ARG and err() == pow2
    # fft.Generator(size) must exist when the polynomial is shifted: BN254's scalar field has 2-adicity 28
    assert call(basis=1, shift=1, size=(1 << 28) + 1) == ARG and "the required root of unity does not exist" in err()
    assert call(polys=_p(a), o=_p(a[1:])) == ARG and err().endswith("the output overlaps an input (inputs are never modified)")
    assert (out == 0).all()

    dv = lib.gmsm_iop_divide_by_x_minus_one
    DV = "gmsm_iop_divide_by_x_minus_one: "
    for h, d in ((None, None), (_p(a), _p(a))):
        assert dv(nohandle, nohandle, h, d, 4, 8, 0, None, _p(out), None) == ARG and err() == DV + one_of("a", "d_a")
        assert dv(nohandle, nohandle, _p(a), None, 4, 8, 0, None, h, d) == ARG and err() == DV + one_of("out", "d_out")
    assert dv(nohandle, nohandle, _p(a), None, 3, 8, 0, None, _p(out), None) == ARG and DV + "unknown basis 3" in err()
    for basis in (1, 2):
        assert dv(nohandle, nohandle, _p(a), None, basis, 8, 0, None, _p(out), None) == ARG and err() == "the basis must be LagrangeCoset"
    assert dv(nohandle, nohandle, _p(a), None, 4, 12, 0, None, _p(out), None) == ARG and DV + "unknown layout 12" in err()
    assert dv(nohandle, nohandle, _p(a), None, 4, 8, 0, None, _p(out), None) == ARG and err() == "unknown fft domain handle"
    assert dv(0, 0, _p(a), None, 4, 16, 1, None, _p(out), None) == ARG and err() == "unknown fft domain handle"
    assert (out == 0).all()


def test_mirror_raises_the_reference_errors(gm):
    iop = gm.iop
    c = gm.CURVES["bn254"]
    z = np.zeros((8, c.fr_limbs), dtype=np.uint64)
    p = iop.NewPolynomial("bn254", z, iop.Form(iop.Lagrange, iop.Regular))
    assert (p.Size(), p.Basis, p.Layout, p.shift) == (8, 2, 8, 0) and p.Coefficients() is z  # not copied
    assert tuple(p)[0] is z and tuple(p)[1:] == (2, 8)  # what the BuildRatio* functions take
    assert p.Shift(3) is p and p.shift == 3
    p.SetSize(4)
    assert p.Size() == 4 and p.Clone().Size() == 4 and p.ShallowClone().Coefficients() is z and p.Clone().Coefficients() is not z

    class FakeDomain:
        handle, Cardinality = 1 << 40, 8
    with pytest.raises(ValueError) as e:
        iop.DivideByXMinusOne(p, (FakeDomain(), FakeDomain()))
    assert str(e.value) == "the basis must be LagrangeCoset"  # ErrMustBeLagrangeCoset, before anything else
    with pytest.raises(ValueError) as e:
        iop.DivideByXMinusOne(iop.NewPolynomial("bn254", z, iop.Form(iop.LagrangeCoset, iop.Regular)), (FakeDomain(), FakeDomain()))
    assert str(e.value) == "unknown fft domain handle"
    with pytest.raises(ValueError) as e:
        p.ToCanonical(FakeDomain())
    assert str(e.value) == "unknown fft domain handle"
    with pytest.raises(ValueError, match="shift 6 is outside 0..5"):
        iop.NewPolynomial("bn254", z, iop.Form(iop.Canonical, iop.Regular)).Shift(6).Evaluate(np.zeros(c.fr_limbs, dtype=np.uint64))
    with pytest.raises(ValueError, match="len must be a power of 2"):
        iop.NewPolynomial("bn254", z[:6], iop.Form(iop.Lagrange, iop.Regular)).Evaluate(np.zeros(c.fr_limbs, dtype=np.uint64))
    for name in ("to_basis_device", "evaluate_device", "divide_by_x_minus_one_device"):
        assert callable(getattr(iop, name))


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
    dev, pure = read(curve, "polynomial_mi355x.go"), read(curve, "polynomial_purego.go")
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    exported = lambda text: re.findall(r"^func (?:\(\w+ \*Polynomial\) )?([A-Z]\w*)\(", text, re.M)
    for text in (dev, pure):
        assert re.search(r"^package iop$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and f'"github.com/consensys/gnark-crypto/{path}/fr/fft"' in text
        assert exported(text) == EXPORTED  # the same exported functions and methods in both builds
    sig = lambda text: re.findall(r"^func ((?:\(\w+ \*Polynomial\) )?[A-Z]\w*\(.*)\{$", text, re.M)
    assert sig(dev) == sig(pure) and len(sig(dev)) == len(EXPORTED)  # ... with the same signatures
    assert 'import "C"' not in pure and "C." not in re.sub(r"//.*", "", pure)
    for ref in ("return p.ToLagrange(d)", "return p.ToCanonical(d)", "return p.ToLagrangeCoset(d)", "return p.Evaluate(x)",
                "return DivideByXMinusOne(a, domains)"):
        assert ref in pure  # the build without the tag calls the reference's methods
    for ref in ("ErrMustBeLagrangeCoset", "gmsmDomain(", "p.grow(", "p.coset.Set("):
        assert ref in dev  # the reference's checks, its grow and its coset stay in the wrapper
    assert "func gmsmDomain(" not in dev  # the handles come from ratios_mi355x.go, as the ratio wrappers obtain them
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert set(SYMBOLS) <= called
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)  # prototypes only: the comments mention the functions too
    lib = gm._lib.load()
    for sym in called:  # every C symbol they call is declared and exported, and called with the prototype's arity
        assert hasattr(lib, sym), sym
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S)
        assert proto, sym
        nargs = 0 if proto.group(1).strip() in ("", "void") else proto.group(1).count(",") + 1
        assert set(call_arities(dev, sym)) == {nargs}, sym


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, ids = CURVES[curve]
    for name in ("polynomial_mi355x.go", "polynomial_purego.go"):
        base = read("bn254", name).replace("ecc/bn254", path).replace("GMSM_BN254_", ids)
        assert base == read(curve, name), name
