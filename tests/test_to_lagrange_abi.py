"""The ToLagrangeG1 entries of the C ABI without a GPU: exported and declared, the argument errors that need no device
return GMSM_ERR_ARG with the reference's texts (len(coeffs) must be a power of 2, the G2 refusal, fr.Generator's order
limit, null pointers, unknown handles), the Python mirror raises them as ValueError, and the Go function
ToLagrangeG1Resident and method (*ResidentProvingKey).ToLagrange exist once in both builds of every curve, identical
across curves, with C calls of the prototypes' arity."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
NEW = ["gmsm_to_lagrange_g1", "gmsm_bases_to_lagrange"]
ERR_POW2 = "len(coeffs) must be a power of 2"  # ToLagrangeG1, ecc/bn254/kzg/utils.go
ERR_G1 = "ToLagrangeG1 is defined for G1 only"
ERR_ROOT = "m is too big: the required root of unity does not exist"
G1 = {"bn254": 0, "bls12_381": 2, "bw6_761": 4}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exported_and_declared(gm):
    lib = gm._lib.load()
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    for sym in NEW:
        assert sym in gm._lib.ABI_SYMBOLS
        assert hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(", header, re.M), sym
        assert getattr(lib, sym).argtypes, sym
    assert "r-torsion" in header[header.index("ToLagrangeG1"):header.index("int gmsm_bases_to_lagrange")]


@pytest.mark.parametrize("curve", sorted(G1))
@pytest.mark.parametrize("n", [0, 3, 6, 1000])
def test_not_a_power_of_two(gm, curve, n):
    L = gm._lib.load()
    pts, out = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    assert L.gmsm_to_lagrange_g1(G1[curve], _p(pts), None, n, None, _p(out), None) == gm._lib.GMSM_ERR_ARG
    assert gm._lib.last_error() == ERR_POW2
    with pytest.raises(ValueError, match=re.escape(ERR_POW2)):
        gm.kzg.ToLagrangeG1(curve, np.zeros((n, 2 * gm.CURVES[curve].fp_limbs), dtype=np.uint64))


@pytest.mark.parametrize("group", [1, 3, 5])
def test_g2_refused(gm, group):
    L = gm._lib.load()
    pts, out = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    assert L.gmsm_to_lagrange_g1(group, _p(pts), None, 2, None, _p(out), None) == gm._lib.GMSM_ERR_ARG
    assert gm._lib.last_error() == ERR_G1
    assert L.gmsm_to_lagrange_g1(99, _p(pts), None, 2, None, _p(out), None) == gm._lib.GMSM_ERR_ARG
    assert gm._lib.last_error() == "unknown group id"


@pytest.mark.parametrize("curve", sorted(G1))
def test_beyond_max_order(gm, curve):
    """fr.Generator(n) fails above the 2-adicity (28 / 32 / 46): checked before any pointer is touched"""
    L = gm._lib.load()
    pts, out = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    n = 1 << (gm.CURVES[curve].fr_max_order + 1)
    assert L.gmsm_to_lagrange_g1(G1[curve], _p(pts), None, n, None, _p(out), None) == gm._lib.GMSM_ERR_ARG
    assert gm._lib.last_error() == ERR_ROOT


def test_null_pointers(gm):
    L = gm._lib.load()
    ARG = gm._lib.GMSM_ERR_ARG
    pts, out = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    assert L.gmsm_to_lagrange_g1(0, None, None, 2, None, _p(out), None) == ARG
    assert "exactly one of coeffs" in gm._lib.last_error()
    assert L.gmsm_to_lagrange_g1(0, _p(pts), _p(pts), 2, None, _p(out), None) == ARG
    assert "exactly one of coeffs" in gm._lib.last_error()
    assert L.gmsm_to_lagrange_g1(0, _p(pts), None, 2, None, None, None) == ARG
    assert "exactly one of out_affine" in gm._lib.last_error()
    assert L.gmsm_to_lagrange_g1(0, _p(pts), None, 2, None, _p(out), _p(out)) == ARG
    assert "exactly one of out_affine" in gm._lib.last_error()


def test_bases_entry_errors(gm):
    L = gm._lib.load()
    ARG = gm._lib.GMSM_ERR_ARG
    h = ctypes.c_uint64(0)
    assert L.gmsm_bases_to_lagrange(12345, 4, ctypes.byref(h)) == ARG  # nothing is registered in this process
    assert gm._lib.last_error() == "unknown bases handle"
    assert L.gmsm_bases_to_lagrange(0, 4, ctypes.byref(h)) == ARG
    assert L.gmsm_bases_to_lagrange(1, 4, None) == ARG
    assert "out_handle is null" in gm._lib.last_error()

    class FakeBases:  # ResidentBases.to_lagrange surfaces the text
        handle, n = 12345, 8
    with pytest.raises(ValueError, match="unknown bases handle"):
        gm.multiexp.ResidentBases.to_lagrange(FakeBases(), 4)


# ---- Go: ToLagrangeG1Resident and (*ResidentProvingKey).ToLagrange in integration/go/<curve>/kzg/
CURVES = {"bn254": ("ecc/bn254", "bn254", "GMSM_BN254_G1"), "bls12-381": ("ecc/bls12-381", "bls12381", "GMSM_BLS12_381_G1"),
          "bw6-761": ("ecc/bw6-761", "bw6761", "GMSM_BW6_761_G1")}


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
def test_go_to_lagrange(gm, curve):
    path, alias, const = CURVES[curve]
    dev, pure = _read(curve, "kzg_mi355x.go"), _read(curve, "kzg_purego.go")
    sigs = [f"func ToLagrangeG1Resident(coeffs []{alias}.G1Affine) ([]{alias}.G1Affine, error)",
            "func (rk *ResidentProvingKey) ToLagrange(size int) (*ResidentProvingKey, error)"]
    for text in (dev, pure):
        for sig in sigs:
            assert text.count(sig) == 1, (curve, sig)
        assert f'"github.com/consensys/gnark-crypto/{path}"' in text
    # the host build is the package's own ToLagrangeG1
    assert "return ToLagrangeG1(coeffs)" in pure and "ToLagrangeG1(rk.host.G1[:size])" in pure
    # the device build: the reference's error text, both entries, a finalizer on the new key
    assert '"len(coeffs) must be a power of 2"' in dev and "bits.OnesCount64(uint64(len(coeffs))) != 1" in dev
    assert '\t"math/bits"\n' in dev
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert set(NEW) <= called
    assert f"C.gmsm_to_lagrange_g1(C.{const}," in dev
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmsm.h")).read(), flags=re.S)
    lib = gm._lib.load()
    for sym in NEW:
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
        assert set(_call_arity(dev, sym)) == {proto.count(",") + 1}, sym
        assert hasattr(lib, sym)
    body = dev[dev.index("func (rk *ResidentProvingKey) ToLagrange("):]
    body = body[:body.index("\n}\n")]
    assert "runtime.SetFinalizer(lk" in body and "runtime.KeepAlive(rk)" in body
    # identical across curves up to the substitutions tests/test_go_stubs.py applies
    strip = lambda t: re.sub(r"//.*", "", t)
    for name in ("kzg_mi355x.go", "kzg_purego.go"):
        base = _read("bn254", name).replace("ecc/bn254", path).replace("bn254.", alias + ".").replace("GMSM_BN254_G1", const)
        assert strip(base) == strip(_read(curve, name)), name
