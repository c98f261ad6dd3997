"""What can be checked of integration/go/<curve>/fflonk/ without a Go toolchain: the two files exclude each other by build
tag, both are `package fflonk` with the same exported API, the device build keeps shplonk's transcript order (gamma over
the extended sets and the digests before the first entry, z over W between the two), every C symbol it calls is declared
in include/gmsm.h and exported by libgmsm.so with the prototype's arity, the exported challenge helper of package shplonk
exists, and the three curve directories are the same files up to the documented substitutions."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
CURVES = {"bn254": ("ecc/bn254", "bn254"), "bls12-381": ("ecc/bls12-381", "bls12381"), "bw6-761": ("ecc/bw6-761", "bw6761")}
API = ("func FoldAndCommitResident(p [][]fr.Element, rk *kzg.ResidentProvingKey) (kzg.Digest, error)",
       "func BatchOpenResident(p [][][]fr.Element, digests []kzg.Digest, points [][]fr.Element, hf hash.Hash, "
       "rk *kzg.ResidentProvingKey, dataTranscript ...[]byte) (OpeningProof, error)")
HELPER = ("func DeriveChallenge(name string, points [][]fr.Element, digests []kzg.Digest, t *fiatshamir.Transcript, "
          "dataTranscript ...[]byte) (fr.Element, error)")


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
def test_fflonk_files(gm, curve):
    path, alias = CURVES[curve]
    dev, pure = read(curve, "fflonk", "fflonk_mi355x.go"), read(curve, "fflonk", "fflonk_purego.go")
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    for text in (dev, pure):
        assert re.search(r"^package fflonk$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and f'"github.com/consensys/gnark-crypto/{path}/kzg"' in text
        for api in API:
            assert text.count(api) == 1
        assert re.findall(r"^func ([A-Z]\w*)\(", text, re.M) == ["FoldAndCommitResident", "BatchOpenResident"]  # the same API in both builds
        assert text.count("rk.Resident()") == 2
    assert "BatchOpen(p, digests, points, hf, pk, dataTranscript...)" in pure and "FoldAndCommit(p, pk)" in pure
    assert "import \"C\"" not in pure
    # the device build: the reference's checks, its divisor and its extended sets, shplonk's challenges, then the entries
    assert "ErrNbPolynomialsNbPoints" in dev and "shplonk.ErrInvalidNumberOfDigests" in dev
    assert "getNextDivisorRMinusOne(len(p[i]))" in dev and "extendSet(points[i], divisors[i])" in dev
    assert 'fiatshamir.NewTranscript(hf, "gamma", "z")' in dev
    assert 'shplonk.DeriveChallenge("gamma", newPoints, digests, fs, dataTranscript...)' in dev
    assert 'shplonk.DeriveChallenge("z", nil, []kzg.Digest{res.SOpeningProof.W}, fs)' in dev
    order = [dev.index(s) for s in ('DeriveChallenge("gamma"', "C.gmsm_fflonk_open_w(", "res.SOpeningProof.W.FromJacobian(&jac)",
                                    'DeriveChallenge("z"', "C.gmsm_fflonk_open_wprime(", "res.SOpeningProof.WPrime.FromJacobian(&jac)")]
    assert order == sorted(order)
    assert f"{alias}.G1Jac" in dev and "res.ClaimedValues[i][j] = claimed[" in dev and "res.SOpeningProof.ClaimedValues[i] = foldedClaimed[" in dev
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert called == {"gmsm_fflonk_fold_commit", "gmsm_fflonk_open_w", "gmsm_fflonk_open_wprime", "gmsm_last_error"}
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)  # prototypes only: the comments mention the functions too
    lib = gm._lib.load()
    for sym in called:
        assert hasattr(lib, sym), sym
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S).group(1)
        nargs = 0 if proto.strip() in ("", "void") else proto.count(",") + 1
        assert set(call_arities(dev, sym)) == {nargs}, sym


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_shplonk_exports_its_challenge(curve):
    path, _ = CURVES[curve]
    text = read(curve, "shplonk", "challenge.go")
    assert not text.startswith("//go:build") and re.search(r"^package shplonk$", text, re.M)  # both builds
    assert text.count(HELPER) == 1 and "return deriveChallenge(name, points, digests, t, dataTranscript...)" in text
    assert re.findall(r"^func ([A-Z]\w*)\(", text, re.M) == ["DeriveChallenge"]
    assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and 'fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"' in text


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, alias = CURVES[curve]
    strip = lambda t: re.sub(r"//.*", "", t)
    for name in (("fflonk", "fflonk_mi355x.go"), ("fflonk", "fflonk_purego.go"), ("shplonk", "challenge.go")):
        base = read("bn254", *name).replace("ecc/bn254", path).replace("bn254.", alias + ".")
        assert strip(base) == strip(read(curve, *name)), name
