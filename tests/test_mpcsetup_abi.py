"""The mpcsetup entries of include/gmsm.h without a device: the three symbols are exported, declared and bound; the header
states the r-torsion precondition; every argument error returns its code and text before any device work and the mirror
(gnark-crypto_amd/mpcsetup.py) raises ValueError with it. And what can be checked of integration/go/<curve>/mpcsetup/
without a Go toolchain: the two files exclude each other by build tag, both are `package mpcsetup` with the same exported
functions, the device build calls exactly the three entries (and gmsm_last_error) with the prototypes' arity, and the
three curve directories are the same files up to the documented substitutions."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
SYMBOLS = ["gmsm_batch_scale", "gmsm_update_monomials", "gmsm_linear_combinations"]
CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
EXPORTED = ["UpdateMonomialsG1Device", "UpdateMonomialsG2Device", "ScaleG1Device", "ScaleG2Device", "LinearCombinationsG1Device",
            "LinearCombinationsG2Device"]
ARG, LEN = 4, 1  # GMSM_ERR_ARG, GMSM_ERR_LEN


def header():
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        return f.read()


def test_symbols_are_exported_declared_and_bound(gm):
    lib = gm._lib.load()
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for sym in SYMBOLS:
        assert sym in gm._lib.ABI_SYMBOLS
        f = getattr(lib, sym)
        assert f.restype is ctypes.c_int
        proto = re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
        assert proto, sym
        assert len(f.argtypes) == proto.group(1).count(",") + 1, sym


def test_header_states_the_precondition():
    h = header()
    doc = re.sub(r"\s*\n \*\s*", " ", h[h.index("mpcsetup updates"):h.index("int gmsm_batch_scale(")])  # the comment's line breaks
    assert "r-torsion" in doc and "Precondition" in doc
    assert "each slice must be of length at least 2" in doc and "lengths mismatch" in doc


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    pts, sc, out = np.zeros((4, 8), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64), np.zeros((4, 8), dtype=np.uint64)
    jac = np.zeros(12, dtype=np.uint64)
    ends = lambda *e: (ctypes.c_size_t * len(e))(*e)
    # gmsm_batch_scale
    assert lib.gmsm_batch_scale(99, _p(pts), None, 4, _p(sc), None, 4, None, _p(out), None) == ARG and "unknown group" in err()
    for ns in (0, 2, 3, 5):
        assert lib.gmsm_batch_scale(0, _p(pts), None, 4, _p(sc), None, ns, None, _p(out), None) == LEN and "n_scalars" in err()
    assert lib.gmsm_batch_scale(0, None, None, 0, None, None, 0, None, None, None) == 0  # n == 0: nothing is touched
    assert lib.gmsm_batch_scale(0, None, None, 0, None, None, 1, None, None, None) == 0
    assert lib.gmsm_batch_scale(0, None, None, 4, _p(sc), None, 4, None, _p(out), None) == ARG and "exactly one of points" in err()
    assert lib.gmsm_batch_scale(0, _p(pts), _p(pts), 4, _p(sc), None, 4, None, _p(out), None) == ARG and "exactly one of points" in err()
    assert lib.gmsm_batch_scale(0, _p(pts), None, 4, None, None, 4, None, _p(out), None) == ARG and "exactly one of scalars" in err()
    assert lib.gmsm_batch_scale(0, _p(pts), None, 4, _p(sc), None, 4, None, None, None) == ARG and "exactly one of out_affine" in err()
    assert lib.gmsm_batch_scale(0, _p(pts), None, 4, _p(sc), None, 4, None, _p(out), _p(out)) == ARG and "exactly one of out_affine" in err()
    # gmsm_update_monomials
    assert lib.gmsm_update_monomials(-1, _p(pts), None, 4, _p(sc), None, _p(out), None) == ARG and "unknown group" in err()
    for n in (0, 1):
        assert lib.gmsm_update_monomials(0, _p(pts), None, n, _p(sc), None, _p(out), None) == ARG and "at least 2 points" in err()
    assert lib.gmsm_update_monomials(0, _p(pts), None, 4, None, None, _p(out), None) == ARG and "r is null" in err()
    assert lib.gmsm_update_monomials(0, None, None, 4, _p(sc), None, _p(out), None) == ARG and "exactly one of points" in err()
    assert lib.gmsm_update_monomials(0, _p(pts), None, 4, _p(sc), None, None, None) == ARG and "exactly one of out_affine" in err()
    # gmsm_linear_combinations
    lc = lib.gmsm_linear_combinations
    assert lc(6, _p(pts), None, 4, ends(4), 1, _p(sc), None, _p(jac), _p(jac)) == ARG and "unknown group" in err()
    assert lc(0, None, None, 4, ends(4), 1, _p(sc), None, _p(jac), _p(jac)) == ARG and "exactly one of points" in err()
    assert lc(0, _p(pts), None, 4, None, 1, _p(sc), None, _p(jac), _p(jac)) == ARG and "must not be null" in err()
    assert lc(0, _p(pts), None, 4, ends(4), 0, _p(sc), None, _p(jac), _p(jac)) == ARG and "must not be null" in err()
    assert lc(0, _p(pts), None, 4, ends(4), 1, None, None, _p(jac), _p(jac)) == ARG and "must not be null" in err()
    assert lc(0, _p(pts), None, 4, ends(4), 1, _p(sc), None, None, _p(jac)) == ARG and "must not be null" in err()
    assert lc(0, _p(pts), None, 4, ends(4), 1, _p(sc), None, _p(jac), None) == ARG and "must not be null" in err()
    assert lc(0, _p(pts), None, 4, ends(2, 2), 2, _p(sc), None, _p(jac), _p(jac)) == ARG and "strictly increasing" in err()
    assert lc(0, _p(pts), None, 4, ends(4, 2), 2, _p(sc), None, _p(jac), _p(jac)) == ARG and "strictly increasing" in err()
    assert lc(0, _p(pts), None, 4, ends(1, 4), 2, _p(sc), None, _p(jac), _p(jac)) == ARG and err() == "each slice must be of length at least 2"
    assert lc(0, _p(pts), None, 4, ends(2, 3), 2, _p(sc), None, _p(jac), _p(jac)) == ARG and err() == "each slice must be of length at least 2"
    assert lc(0, _p(pts), None, 4, ends(2), 1, _p(sc), None, _p(jac), _p(jac)) == ARG and err() == "lengths mismatch"
    assert lc(0, _p(pts), None, 4, ends(2, 5), 2, _p(sc), None, _p(jac), _p(jac)) == ARG and err() == "lengths mismatch"


def test_mirror_raises_value_error(gm):
    m = gm.mpcsetup
    c = gm.CURVES["bn254"]
    pts, one = np.zeros((4, 2 * c.fp_limbs), dtype=np.uint64), np.zeros(c.fr_limbs, dtype=np.uint64)
    assert m.BatchScaleG1("bn254", pts[:0], np.zeros((0, c.fr_limbs), dtype=np.uint64)).shape == (0, 2 * c.fp_limbs)
    with pytest.raises(ValueError, match="n_scalars"):
        m.BatchScaleG1("bn254", pts, np.zeros((3, c.fr_limbs), dtype=np.uint64))
    with pytest.raises(ValueError, match="n_scalars"):
        m.BatchScaleG2("bn254", np.zeros((4, 4 * c.fp_limbs), dtype=np.uint64), np.zeros((2, c.fr_limbs), dtype=np.uint64))
    for f in (m.UpdateMonomialsG1, m.UpdateMonomialsG2):
        with pytest.raises(ValueError, match="at least 2 points"):
            f("bn254", pts[:0], one)
    with pytest.raises(ValueError, match="at least 2 points"):
        m.UpdateMonomialsG1("bn254", pts[:1], one)
    with pytest.raises(ValueError, match="lengths mismatch"):
        m.linearCombinationsG1("bn254", pts, one, [2])
    with pytest.raises(ValueError, match="each slice must be of length at least 2"):
        m.linearCombinationsG1("bn254", pts, one, [3, 4])
    with pytest.raises(ValueError, match="strictly increasing"):
        m.linearCombinationsG2("bn254", np.zeros((4, 4 * c.fp_limbs), dtype=np.uint64), one, [4, 4])
    with pytest.raises(ValueError, match="must not be null"):
        m.linearCombinationsG1("bn254", pts, one, [])
    for name in ("batch_scale_device", "update_monomials_device", "linear_combinations_device"):
        assert callable(getattr(m, name))


# ---- the Go files
def read(curve, name):
    with open(os.path.join(GO, curve, "mpcsetup", name)) as f:
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
    dev, pure = read(curve, "mpcsetup_mi355x.go"), read(curve, "mpcsetup_purego.go")
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    for text in (dev, pure):
        assert re.search(r"^package mpcsetup$", text, re.M)
        assert f'curve "github.com/consensys/gnark-crypto/{path}"' in text and f'"github.com/consensys/gnark-crypto/{path}/fr"' in text
        assert re.findall(r"^func ([A-Z]\w*)\(", text, re.M) == EXPORTED  # the same exported functions in both builds
    sig = lambda text: re.findall(r"^func ([A-Z]\w*\(.*)\{$", text, re.M)
    assert sig(dev) == sig(pure)  # ... with the same signatures
    assert 'import "C"' not in pure and "C." not in re.sub(r"//.*", "", pure)
    for ref in ("UpdateMonomialsG1(A, r)", "linearCombinationsG1(", "linearCombinationsG2(", ".ScalarMultiplication("):
        assert ref in pure
    assert f"C.{ids}G1" in dev and f"C.{ids}G2" in dev
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert called == set(SYMBOLS) | {"gmsm_last_error"}
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)  # prototypes only: the comments mention the functions too
    lib = gm._lib.load()
    for sym in called:
        assert hasattr(lib, sym), sym
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S).group(1)
        nargs = 0 if proto.strip() in ("", "void") else proto.count(",") + 1
        assert set(call_arities(dev, sym)) == {nargs}, sym


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, ids = CURVES[curve]
    for name in ("mpcsetup_mi355x.go", "mpcsetup_purego.go"):
        base = read("bn254", name).replace("ecc/bn254", path).replace("GMSM_BN254_", ids)
        assert base == read(curve, name), name
