"""What can be checked of integration/go/<curve>/fr/fri/ without a Go toolchain: the device and the plain file exclude each other by
build tag, both are `package fri` with the same exported API, the plain build calls the reference's own prover over mimc.NewMiMC(),
every C symbol the device build calls is declared in include/gmsm.h and exported by libgmsm.so with the prototype's arity, and
the three curve directories are the same files up to the documented substitutions."""
import os
import re

import pytest

from test_go_fflonk_stubs import call_arities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
FILES = ("fri_mi355x.go", "fri_purego.go")
API = ("func BuildProofOfProximityDevice(size uint64, p []fr.Element) (ProofOfProximity, error)",
       "func OpenDevice(size uint64, p []fr.Element, position uint64) (OpeningProof, error)")
DEVICE_CALLS = {"gmsm_fft_domain_new", "gmsm_fft_domain_release", "gmsm_fri_commit", "gmsm_fri_root", "gmsm_fri_fold", "gmsm_fri_query",
                "gmsm_fri_release", "gmsm_last_error"}


def read(curve, name):
    with open(os.path.join(GO, curve, "fr", "fri", name)) as f:
        return f.read()


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_fri_files(gm, curve):
    path, prefix = CURVES[curve]
    assert sorted(os.listdir(os.path.join(GO, curve, "fr", "fri"))) == sorted(FILES)
    texts = {name: read(curve, name) for name in FILES}
    for name, text in texts.items():
        tag = "//go:build mi355x\n" if name.endswith("_mi355x.go") else "//go:build !mi355x\n"
        assert text.startswith(tag)  # file-level, mutually exclusive
        assert re.search(r"^package fri$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text and f'"github.com/consensys/gnark-crypto/{path}/fr/mimc"' in text
        for api in API:  # the same API in both builds
            assert text.count(api) == 1
        assert re.findall(r"^func ([A-Z]\w*)\(", text, re.M) == ["BuildProofOfProximityDevice", "OpenDevice"]
        assert text.count("var ErrDeviceSize = errors.New(") == 1
    pure, dev = texts["fri_purego.go"], texts["fri_mi355x.go"]
    assert 'import "C"' not in pure
    assert "RADIX_2_FRI.New(size, mimc.NewMiMC()).BuildProofOfProximity(p)" in pure and "RADIX_2_FRI.New(size, mimc.NewMiMC()).Open(p, position)" in pure
    assert f"const gmsmG1 = C.int(C.{prefix}G1)" in dev and '#include "gmsm.h"' in dev
    assert set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev)) == DEVICE_CALLS
    # the reference's transcript and its own position arithmetic, not copies of them
    assert "fiatshamir.NewTranscript(mimc.NewMiMC(), xis...)" in dev and "deriveQueriesPositions(" in dev and "convertCanonicalSorted(" in dev
    # the neighbour's proof: its leaf and the sum of the queried leaf, which the tree holds already
    assert "[][]byte{pairs[2*i+1-c].Marshal(), sums[i].Marshal()}" in dev
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)  # prototypes only: the comments mention the functions too
    lib = gm._lib.load()
    for sym in DEVICE_CALLS:
        assert hasattr(lib, sym), sym
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S).group(1)
        nargs = 0 if proto.strip() in ("", "void") else proto.count(",") + 1
        assert set(call_arities(dev, sym)) == {nargs}, sym


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, prefix = CURVES[curve]
    strip = lambda t: re.sub(r"//.*", "", t)
    for name in FILES:
        base = read("bn254", name).replace("ecc/bn254", path).replace("GMSM_BN254_", prefix)
        assert strip(base) == strip(read(curve, name)), name


def test_readme_has_the_row():
    with open(os.path.join(GO, "README.md")) as f:
        text = f.read()
    for word in ("fr/fri/fri_mi355x.go", "BuildProofOfProximityDevice", "OpenDevice", "gmsm_fri_commit", "gmsm_fri_query"):
        assert word in text, word
