"""The fr.BatchInvert / iop ratio entries of include/gmsm.h without a device: the three symbols are exported, declared with
the stated arity and bound; every argument error the host can decide returns GMSM_ERR_ARG with its text before any device
work; the mirror (gnark-crypto_amd/iop.py) raises ValueError with the reference's texts. And what can be checked of
integration/go/<curve>/iop/ without a Go toolchain: the two files exclude each other by build tag, both are `package iop`
with the same exported functions and signatures, the device build calls only entries the header declares and the library
exports, with the prototypes' arity, and the three curve directories are the same files up to the documented substitutions."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
SYMBOLS = {"gmsm_fr_batch_invert": 7, "gmsm_iop_ratio_copy_constraint": 14, "gmsm_iop_ratio_shuffled": 14}
CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
EXPORTED = ["BuildRatioCopyConstraintDevice", "BuildRatioShuffledVectorsDevice", "BatchInvertDevice"]
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
    doc = re.sub(r"\s*\n \*\s*", " ", h[h.index("fr.BatchInvert (ecc"):h.index("int gmsm_fr_batch_invert(")])
    assert "LAGRANGE basis" in doc and "stays with the caller" in doc  # the C entries take Lagrange only
    assert "the reference panics there" in doc and "is outside [0, m n)" in doc
    assert "never built" in doc  # the support is not materialised


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    a, out = np.zeros((4, 4), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64)
    inv = lib.gmsm_fr_batch_invert
    assert inv(99, _p(a), None, 4, None, _p(out), None) == ARG and "unknown group" in err()
    for gid in range(6):
        assert inv(gid, None, None, 0, None, None, None) == 0  # n == 0: GMSM_OK, nothing is touched
    assert inv(0, None, None, 4, None, _p(out), None) == ARG and "exactly one of a (host) / d_a" in err()
    assert inv(0, _p(a), _p(a), 4, None, _p(out), None) == ARG and "exactly one of a (host) / d_a" in err()
    assert inv(0, _p(a), None, 4, None, None, None) == ARG and "exactly one of out (host) / d_out" in err()
    assert inv(0, _p(a), None, 4, None, _p(out), _p(out)) == ARG and "exactly one of out (host) / d_out" in err()

    ent, perm = np.zeros((8, 4), dtype=np.uint64), np.arange(8, dtype=np.int64)
    lay = np.array([8, 16], dtype=np.uint32)
    lp = lambda x: x.ctypes.data_as(U32P)
    beta = np.zeros(4, dtype=np.uint64)
    cc, sv = lib.gmsm_iop_ratio_copy_constraint, lib.gmsm_iop_ratio_shuffled
    nohandle = 1 << 40
    # in the order of the checks: the count, the expected form, the output pair, the handle
    assert cc(nohandle, _p(ent), None, 0, lp(lay), _p(perm), None, _p(beta), _p(beta), 2, 8, None, _p(out), None) == ARG and "m == 0" in err()
    assert sv(nohandle, _p(ent), None, _p(ent), None, 0, lp(lay), lp(lay), _p(beta), 2, 8, None, _p(out), None) == ARG and "m == 0" in err()
    for basis in (0, 3, 8):
        assert cc(nohandle, _p(ent), None, 2, lp(lay), _p(perm), None, _p(beta), _p(beta), basis, 8, None, _p(out), None) == ARG
        assert f"unknown basis {basis}" in err()
        assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), lp(lay), _p(beta), basis, 8, None, _p(out), None) == ARG
        assert f"unknown basis {basis}" in err()
    for layout in (0, 1, 24):
        assert cc(nohandle, _p(ent), None, 2, lp(lay), _p(perm), None, _p(beta), _p(beta), 2, layout, None, _p(out), None) == ARG
        assert f"unknown layout {layout}" in err()
        assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), lp(lay), _p(beta), 4, layout, None, _p(out), None) == ARG
        assert f"unknown layout {layout}" in err()
    assert cc(nohandle, _p(ent), None, 2, lp(lay), _p(perm), None, _p(beta), _p(beta), 2, 8, None, None, None) == ARG
    assert "exactly one of out (host) / d_out" in err()
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), lp(lay), _p(beta), 2, 8, None, _p(out), _p(out)) == ARG
    assert "exactly one of out (host) / d_out" in err()
    # the entries' own pointers, pairs and layout values: before the handle is looked at, each with its text
    CC, SV = "gmsm_iop_ratio_copy_constraint: ", "gmsm_iop_ratio_shuffled: "
    bad_lay = np.array([8, 4], dtype=np.uint32)
    tail = (2, 8, None, _p(out), None)
    assert cc(nohandle, _p(ent), None, 2, None, _p(perm), None, _p(beta), _p(beta), *tail) == ARG and err() == CC + "layouts is null"
    assert cc(nohandle, _p(ent), None, 2, lp(bad_lay), _p(perm), None, _p(beta), _p(beta), *tail) == ARG
    assert err() == CC + "layouts[1] = 4 is no layout (8 Regular, 16 BitReverse)"
    assert cc(nohandle, _p(ent), None, 2, lp(lay), _p(perm), None, None, _p(beta), *tail) == ARG and err() == CC + "beta and gamma must not be null"
    assert cc(nohandle, _p(ent), None, 2, lp(lay), _p(perm), None, _p(beta), None, *tail) == ARG and err() == CC + "beta and gamma must not be null"
    one_of = lambda h, d: f"give exactly one of {h} (host) / {d} (device)"
    for e, de in ((None, None), (_p(ent), _p(ent))):
        assert cc(nohandle, e, de, 2, lp(lay), _p(perm), None, _p(beta), _p(beta), *tail) == ARG and err() == CC + one_of("entries", "d_entries")
    for q, dq in ((None, None), (_p(perm), _p(perm))):
        assert cc(nohandle, _p(ent), None, 2, lp(lay), q, dq, _p(beta), _p(beta), *tail) == ARG and err() == CC + one_of("perm", "d_perm")
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, None, lp(lay), _p(beta), *tail) == ARG and err() == SV + "num_layouts is null"
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), None, _p(beta), *tail) == ARG and err() == SV + "den_layouts is null"
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(bad_lay), lp(lay), _p(beta), *tail) == ARG
    assert err() == SV + "num_layouts[1] = 4 is no layout (8 Regular, 16 BitReverse)"
    bad0 = np.array([0, 16], dtype=np.uint32)
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), lp(bad0), _p(beta), *tail) == ARG
    assert err() == SV + "den_layouts[0] = 0 is no layout (8 Regular, 16 BitReverse)"
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), lp(lay), None, *tail) == ARG and err() == SV + "beta must not be null"
    for a, da in ((None, None), (_p(ent), _p(ent))):
        assert sv(nohandle, a, da, _p(ent), None, 2, lp(lay), lp(lay), _p(beta), *tail) == ARG and err() == SV + one_of("num", "d_num")
        assert sv(nohandle, _p(ent), None, a, da, 2, lp(lay), lp(lay), _p(beta), *tail) == ARG and err() == SV + one_of("den", "d_den")
    # only then the handle (the overlap of the output with an input needs the domain's size: tests/test_gpu_iop.py)
    assert cc(nohandle, _p(ent), None, 2, lp(lay), _p(perm), None, _p(beta), _p(beta), 2, 8, None, _p(out), None) == ARG
    assert err() == "unknown fft domain handle"
    assert cc(0, _p(ent), None, 2, lp(lay), _p(perm), None, _p(beta), _p(beta), 1, 16, None, _p(out), None) == ARG
    assert err() == "unknown fft domain handle"
    assert sv(nohandle, _p(ent), None, _p(ent), None, 2, lp(lay), lp(lay), _p(beta), 2, 8, None, _p(out), None) == ARG
    assert err() == "unknown fft domain handle"


def test_mirror_raises_the_reference_errors(gm):
    iop = gm.iop
    assert (iop.Canonical, iop.Lagrange, iop.LagrangeCoset, iop.Regular, iop.BitReverse) == (1, 2, 4, 8, 16)  # polynomial.go:20-34
    assert (iop.Basis.LagrangeCoset, iop.Layout.BitReverse) == (4, 16)
    c = gm.CURVES["bn254"]
    form = iop.Form(iop.Lagrange, iop.Regular)
    v = lambda n: (np.zeros((n, c.fr_limbs), dtype=np.uint64), iop.Lagrange, iop.Regular)
    z = np.zeros(c.fr_limbs, dtype=np.uint64)

    class FakeDomain:
        Cardinality = 16
    with pytest.raises(ValueError) as e:
        iop.BuildRatioShuffledVectors("bn254", [v(8), v(8)], [v(8)], z, form)
    assert str(e.value) == "the number of polynomials in the denominator and the numerator must be the same"
    with pytest.raises(ValueError) as e:
        iop.BuildRatioShuffledVectors("bn254", [v(8), v(4)], [v(8), v(8)], z, form)
    assert str(e.value) == "the sizes of the polynomial must be the same as the size of the domain"
    with pytest.raises(ValueError) as e:
        iop.BuildRatioCopyConstraint("bn254", [v(8), v(16)], np.arange(24), z, z, form)
    assert str(e.value) == "the sizes of the polynomial must be the same as the size of the domain"
    with pytest.raises(ValueError) as e:
        iop.BuildRatioCopyConstraint("bn254", [v(6), v(6)], np.arange(12), z, z, form)
    assert str(e.value) == "the size of the polynomials must be a power of two"
    with pytest.raises(ValueError) as e:
        iop.BuildRatioShuffledVectors("bn254", [v(12)], [v(12)], z, form)
    assert str(e.value) == "the size of the polynomials must be a power of two"
    with pytest.raises(ValueError) as e:
        iop.BuildRatioCopyConstraint("bn254", [v(8)], np.arange(8), z, z, form, FakeDomain())
    assert str(e.value) == "the size of the domain must be consistent with the size of the polynomials"
    with pytest.raises(ValueError, match="m == 0"):
        iop.BuildRatioCopyConstraint("bn254", [], np.arange(0), z, z, form)
    assert iop.BatchInvert("bn254", np.zeros((0, c.fr_limbs), dtype=np.uint64)).shape == (0, c.fr_limbs)
    for name in ("batch_invert_device", "build_ratio_copy_constraint_device", "build_ratio_shuffled_vectors_device"):
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
    dev, pure = read(curve, "ratios_mi355x.go"), read(curve, "ratios_purego.go")
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    for text in (dev, pure):
        assert re.search(r"^package iop$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and f'"github.com/consensys/gnark-crypto/{path}/fr/fft"' in text
        assert re.findall(r"^func ([A-Z]\w*)\(", text, re.M) == EXPORTED  # the same exported functions in both builds
    sig = lambda text: re.findall(r"^func ([A-Z]\w*\(.*)\{$", text, re.M)
    assert sig(dev) == sig(pure)  # ... with the same signatures
    assert 'import "C"' not in pure and "C." not in re.sub(r"//.*", "", pure)
    for ref in ("return BuildRatioCopyConstraint(", "return BuildRatioShuffledVectors(", "return fr.BatchInvert("):
        assert ref in pure  # the build without the tag calls the reference's functions
    for ref in ("checkSize(", "buildDomain(", ".ToLagrange(domain)", "ErrNumberPolynomials"):
        assert ref in dev  # the reference's checks and its ToLagrange stay in the wrapper
    assert f"C.{ids}G1" in dev
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
    for name in ("ratios_mi355x.go", "ratios_purego.go"):
        base = read("bn254", name).replace("ecc/bn254", path).replace("GMSM_BN254_", ids)
        assert base == read(curve, name), name
