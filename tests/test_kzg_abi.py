"""The KZG opening entries of the C ABI without a GPU: exported and declared, the argument errors that need no device
return the documented codes and the reference's texts, and the Go methods Open / BatchOpenSinglePoint of the resident
proving key exist once in both builds of every curve, identical across curves, with C calls of the prototypes' arity."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
NEW = ["gmsm_poly_eval", "gmsm_poly_div_x_minus_a", "gmsm_kzg_open", "gmsm_kzg_open_folded"]
ERR_SIZE = "invalid polynomial size (larger than SRS or == 0)"  # ErrInvalidPolynomialSize, ecc/bn254/kzg/kzg.go


def test_symbols_exported_and_declared(gm):
    lib = gm._lib.load()
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    for sym in NEW:
        assert sym in gm._lib.ABI_SYMBOLS
        assert hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(", header, re.M), sym
        assert getattr(lib, sym).argtypes, sym


def _u64(n):
    return np.zeros(n, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sizes(*lens):
    return (ctypes.c_size_t * len(lens))(*lens)


@pytest.mark.parametrize("n", [0, 1])
def test_open_refuses_degenerate_sizes(gm, n):
    L = gm._lib.load()
    poly, point, claimed, jac = _u64(8), _u64(4), _u64(4), _u64(12)
    rc = L.gmsm_kzg_open(1, _p(poly) if n else None, None, n, _p(point), None, _p(claimed), _p(jac))
    assert rc == gm._lib.GMSM_ERR_ARG and gm._lib.last_error() == ERR_SIZE


def test_open_folded_refuses_sizes(gm):
    L = gm._lib.load()
    polys, point, gamma, jac = _u64(16), _u64(4), _u64(4), _u64(12)
    for lens in ((1,), (1, 1, 1), (3, 0, 2)):  # largest member of length 1; an empty member
        rc = L.gmsm_kzg_open_folded(1, _p(polys), None, _sizes(*lens), len(lens), _p(point), _p(gamma), None, _p(jac))
        assert rc == gm._lib.GMSM_ERR_ARG and gm._lib.last_error() == ERR_SIZE, lens
    rc = L.gmsm_kzg_open_folded(1, _p(polys), None, _sizes(2), 0, _p(point), _p(gamma), None, _p(jac))
    assert rc == gm._lib.GMSM_ERR_ARG


def test_open_argument_errors(gm):
    L = gm._lib.load()
    poly, point, claimed, jac = _u64(16), _u64(4), _u64(4), _u64(12)
    ARG = gm._lib.GMSM_ERR_ARG
    # unknown handle (nothing is registered in this process)
    assert L.gmsm_kzg_open(12345, _p(poly), None, 4, _p(point), None, _p(claimed), _p(jac)) == ARG
    assert gm._lib.last_error() == "unknown bases handle"
    # neither / both of host and device polynomial
    assert L.gmsm_kzg_open(1, None, None, 4, _p(point), None, _p(claimed), _p(jac)) == ARG
    assert "exactly one of" in gm._lib.last_error()
    assert L.gmsm_kzg_open(1, _p(poly), _p(poly), 4, _p(point), None, _p(claimed), _p(jac)) == ARG
    # null point / outputs, outputs aliasing
    assert L.gmsm_kzg_open(1, _p(poly), None, 4, None, None, _p(claimed), _p(jac)) == ARG
    assert L.gmsm_kzg_open(1, _p(poly), None, 4, _p(point), None, None, _p(jac)) == ARG
    assert L.gmsm_kzg_open(1, _p(poly), None, 4, _p(point), None, _p(jac), _p(jac)) == ARG
    assert L.gmsm_kzg_open(1, _p(poly), None, 4, _p(point), None, _p(claimed), _p(poly)) == ARG
    assert "aliases" in gm._lib.last_error()
    gamma = _u64(4)
    assert L.gmsm_kzg_open_folded(1, _p(poly), None, _sizes(2, 2), 2, _p(point), None, None, _p(jac)) == ARG  # gamma missing


def test_poly_entries_argument_errors(gm):
    L = gm._lib.load()
    ARG = gm._lib.GMSM_ERR_ARG
    poly, point, h, value = _u64(16), _u64(4), _u64(16), _u64(4)
    assert L.gmsm_poly_div_x_minus_a(0, _p(poly), None, 0, _p(point), None, _p(h), None, _p(value)) == ARG
    assert "n == 0" in gm._lib.last_error()
    assert L.gmsm_poly_div_x_minus_a(0, _p(poly), None, 4, _p(point), None, None, None, _p(value)) == ARG  # no h output
    assert L.gmsm_poly_div_x_minus_a(0, _p(poly), None, 4, _p(point), None, _p(poly), None, _p(value)) == ARG  # h over the input
    assert "aliases" in gm._lib.last_error()
    assert L.gmsm_poly_div_x_minus_a(0, _p(poly), None, 4, None, None, _p(h), None, _p(value)) == ARG
    assert L.gmsm_poly_div_x_minus_a(99, _p(poly), None, 4, _p(point), None, _p(h), None, _p(value)) == ARG
    assert gm._lib.last_error() == "unknown group id"
    out = _u64(8)
    assert L.gmsm_poly_eval(0, _p(poly), None, _sizes(2, 0), 2, _p(point), None, _p(out)) == ARG
    assert "empty" in gm._lib.last_error()
    assert L.gmsm_poly_eval(0, None, None, _sizes(2), 1, _p(point), None, _p(out)) == ARG
    assert L.gmsm_poly_eval(0, _p(poly), None, _sizes(2), 1, _p(point), None, _p(poly)) == ARG
    assert L.gmsm_poly_eval(0, _p(poly), None, _sizes(2), 0, _p(point), None, _p(out)) == gm._lib.GMSM_OK  # nothing to do


def test_python_mirror_raises_reference_errors(gm):
    """kzg.Open / BatchOpenSinglePoint surface the library's text (no handle is needed to reach the size checks)."""
    class FakeBases:
        handle = 1
        group = gm.G1Affine("bn254")
    with pytest.raises(ValueError, match=re.escape(ERR_SIZE)):
        gm.kzg.Open(np.zeros((1, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), FakeBases())
    with pytest.raises(ValueError, match=re.escape(ERR_SIZE)):
        gm.kzg.BatchOpenSinglePoint([np.zeros((1, 4), dtype=np.uint64)] * 3, np.zeros(4, dtype=np.uint64),
                                    np.zeros(4, dtype=np.uint64), FakeBases())
    with pytest.raises(ValueError, match="n == 0"):
        gm.kzg.DividePolyByXMinusA("bn254", np.zeros((0, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64))


# ---- Go: (*ResidentProvingKey).Open / BatchOpenSinglePoint in integration/go/<curve>/kzg/
CURVES = {"bn254": ("ecc/bn254", "bn254", "GMSM_BN254_G1"), "bls12-381": ("ecc/bls12-381", "bls12381", "GMSM_BLS12_381_G1"),
          "bw6-761": ("ecc/bw6-761", "bw6761", "GMSM_BW6_761_G1")}
SIGS = ["func (rk *ResidentProvingKey) Open(p []fr.Element, point fr.Element) (OpeningProof, error)",
        "func (rk *ResidentProvingKey) BatchOpenSinglePoint(polynomials [][]fr.Element, digests []Digest, point fr.Element, "
        "hf hash.Hash, dataTranscript ...[]byte) (BatchOpeningProof, error)"]


def _read(curve, name):
    with open(os.path.join(GO, curve, "kzg", name)) as f:
        return f.read()


def _call_arity(text, sym):
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
def test_go_open_methods(gm, curve):
    path, alias, const = CURVES[curve]
    dev, pure = _read(curve, "kzg_mi355x.go"), _read(curve, "kzg_purego.go")
    for text in (dev, pure):
        for sig in SIGS:
            assert text.count(sig) == 1, (curve, sig)
        assert '\t"hash"\n' in text
    assert "Open(p, point, rk.host)" in pure and "BatchOpenSinglePoint(polynomials, digests, point, hf, rk.host, dataTranscript...)" in pure
    # the device build: the reference's checks, the host fallback below MinDevicePoints, the challenge from deriveGamma
    assert "ErrInvalidNbDigests" in dev and "deriveGamma(point, digests, res.ClaimedValues, hf, dataTranscript...)" in dev
    assert "Open(p, point, rk.host)" in dev and "BatchOpenSinglePoint(polynomials, digests, point, hf, rk.host, dataTranscript...)" in dev
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert {"gmsm_kzg_open", "gmsm_poly_eval", "gmsm_kzg_open_folded"} <= called
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmsm.h")).read(), flags=re.S)
    lib = gm._lib.load()
    for sym in ("gmsm_kzg_open", "gmsm_poly_eval", "gmsm_kzg_open_folded"):
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
        assert set(_call_arity(dev, sym)) == {proto.count(",") + 1}, sym
        assert hasattr(lib, sym)
    # identical across curves up to the substitutions tests/test_go_stubs.py applies
    strip = lambda t: re.sub(r"//.*", "", t)
    for name in ("kzg_mi355x.go", "kzg_purego.go"):
        base = _read("bn254", name).replace("ecc/bn254", path).replace("bn254.", alias + ".").replace("GMSM_BN254_G1", const)
        assert strip(base) == strip(_read(curve, name)), name
