"""What can be checked of integration/go/<curve>/shplonk/ without a Go toolchain: the two files exclude each other by
build tag, both are `package shplonk` with the same exported API, every C symbol the device build calls is declared in
include/gmsm.h and exported by libgmsm.so with the prototype's arity, the kzg accessor it needs exists once in both kzg
builds, and the three curve directories are the same files up to the documented substitutions."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
CURVES = {"bn254": ("ecc/bn254", "bn254"), "bls12-381": ("ecc/bls12-381", "bls12381"), "bw6-761": ("ecc/bw6-761", "bw6761")}
API = ("func BatchOpenResident(polynomials [][]fr.Element, digests []kzg.Digest, points [][]fr.Element, hf hash.Hash, "
       "rk *kzg.ResidentProvingKey, dataTranscript ...[]byte) (OpeningProof, error)")
ACCESSOR = "func (rk *ResidentProvingKey) Resident() (uint64, ProvingKey)"


def read(curve, *name):
    with open(os.path.join(GO, curve, *name)) as f:
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
def test_shplonk_files(gm, curve):
    path, alias = CURVES[curve]
    dev, pure = read(curve, "shplonk", "shplonk_mi355x.go"), read(curve, "shplonk", "shplonk_purego.go")
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    for text in (dev, pure):
        assert re.search(r"^package shplonk$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and f'"github.com/consensys/gnark-crypto/{path}/kzg"' in text
        assert text.count(API) == 1
        assert re.findall(r"^func ([A-Z]\w*)\(", text, re.M) == ["BatchOpenResident"]  # the same exported API in both builds
        assert "rk.Resident()" in text
    assert "BatchOpen(polynomials, digests, points, hf, pk, dataTranscript...)" in pure and "import \"C\"" not in pure
    # the device build: the reference's checks and its own challenges, then the two entries
    assert "ErrInvalidNumberOfPoints" in dev and "ErrInvalidNumberOfDigests" in dev
    assert 'deriveChallenge("gamma", points, digests, fs, dataTranscript...)' in dev
    assert 'deriveChallenge("z", nil, []kzg.Digest{res.W}, fs)' in dev
    assert dev.index("C.gmsm_shplonk_open_w(") < dev.index('deriveChallenge("z"') < dev.index("C.gmsm_shplonk_open_wprime(")
    assert f"{alias}.G1Jac" in dev and "res.W.FromJacobian(&jac)" in dev and "res.WPrime.FromJacobian(&jac)" in dev
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert called == {"gmsm_shplonk_open_w", "gmsm_shplonk_open_wprime", "gmsm_last_error"}
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)  # prototypes only: the comments mention the functions too
    lib = gm._lib.load()
    for sym in called:
        assert hasattr(lib, sym), sym
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S).group(1)
        nargs = 0 if proto.strip() in ("", "void") else proto.count(",") + 1
        assert set(call_arities(dev, sym)) == {nargs}, sym


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_kzg_accessor_in_both_builds(curve):
    dev, pure = read(curve, "kzg", "kzg_mi355x.go"), read(curve, "kzg", "kzg_purego.go")
    for text in (dev, pure):
        assert text.count(ACCESSOR) == 1
    assert "return uint64(rk.handle), rk.host" in dev and "return 0, rk.host" in pure


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, alias = CURVES[curve]
    strip = lambda t: re.sub(r"//.*", "", t)
    for name in ("shplonk_mi355x.go", "shplonk_purego.go"):
        base = read("bn254", "shplonk", name).replace("ecc/bn254", path).replace("bn254.", alias + ".")
        assert strip(base) == strip(read(curve, "shplonk", name)), name
