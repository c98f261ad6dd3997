"""What can be checked of integration/go/<curve>/fr/mimc/ without a Go toolchain: the device and the plain files exclude each
other by build tag, all are `package mimc` with the same exported API, the plain build loops over NewMiMC() and
merkletree.New, every C symbol the device build calls is declared in include/gmsm.h and exported by libgmsm.so with the
prototype's arity, and the three curve directories are the same files up to the documented substitutions."""
import os
import re

import pytest

from test_go_fflonk_stubs import call_arities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "integration", "go")
CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
FILES = ("mimc_mi355x.go", "mimc_purego.go", "merkle_mi355x.go", "merkle_purego.go")
BATCH_API = "func SumBatchDevice(msgs []fr.Element, msgLen int) ([]fr.Element, error)"
TREE_API = ("func NewDeviceTree(leaves []fr.Element, leafLen int) (*DeviceTree, error)",
            "func (t *DeviceTree) NumLeaves() uint64",
            "func (t *DeviceTree) Root() ([]byte, error)",
            "func (t *DeviceTree) Prove(indices []uint64) ([][][]byte, error)",
            "func (t *DeviceTree) Release() error")


def read(curve, name):
    with open(os.path.join(GO, curve, "fr", "mimc", name)) as f:
        return f.read()


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_mimc_files(gm, curve):
    path, prefix = CURVES[curve]
    assert sorted(os.listdir(os.path.join(GO, curve, "fr", "mimc"))) == sorted(FILES)
    texts = {name: read(curve, name) for name in FILES}
    for name, text in texts.items():
        tag = "//go:build mi355x\n" if name.endswith("_mi355x.go") else "//go:build !mi355x\n"
        assert text.startswith(tag)  # file-level, mutually exclusive
        assert re.search(r"^package mimc$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr"' in text
    for kind in ("mi355x", "purego"):  # the same API in both builds
        batch, tree = texts[f"mimc_{kind}.go"], texts[f"merkle_{kind}.go"]
        assert batch.count(BATCH_API) == 1 and re.findall(r"^func ([A-Z]\w*)\(", batch, re.M) == ["SumBatchDevice"]
        assert batch.count("var ErrBatchShape = errors.New(") == 1
        for api in TREE_API:
            assert tree.count(api) == 1
        assert re.findall(r"^func ([A-Z]\w*)\(", tree, re.M) == ["NewDeviceTree"]
        assert re.findall(r"^func \(t \*DeviceTree\) ([A-Z]\w*)\(", tree, re.M) == ["NumLeaves", "Root", "Prove", "Release"]
        assert tree.count("type DeviceTree struct {") == 1
    pure_batch, pure_tree = texts["mimc_purego.go"], texts["merkle_purego.go"]
    assert 'import "C"' not in pure_batch + pure_tree
    assert "h := NewMiMC()" in pure_batch and "h.Write(b[:])" in pure_batch and "SetBytes(h.Sum(nil))" in pure_batch
    assert '"github.com/consensys/gnark-crypto/accumulator/merkletree"' in pure_tree
    assert pure_tree.count("tree := merkletree.New(NewMiMC())") == 2 and "tree.SetIndex(index)" in pure_tree and "tree.Prove()" in pure_tree
    dev_batch, dev_tree = texts["mimc_mi355x.go"], texts["merkle_mi355x.go"]
    assert f"const gmsmG1 = C.int(C.{prefix}G1)" in dev_batch and '#include "gmsm.h"' in dev_batch and '#include "gmsm.h"' in dev_tree
    assert set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev_batch)) == {"gmsm_mimc_sum_batch", "gmsm_last_error"}
    assert set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev_tree)) == {"gmsm_merkle_new", "gmsm_merkle_info", "gmsm_merkle_root", "gmsm_merkle_prove",
                                                                  "gmsm_merkle_release"}
    # the proof set: the leaf's data first, then counts[j] siblings of the path's depth slots
    assert "res[j] = append(res[j], data)" in dev_tree and "siblings[j*t.depth : j*t.depth+int(counts[j])]" in dev_tree
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)  # prototypes only: the comments mention the functions too
    lib = gm._lib.load()
    for text in (dev_batch, dev_tree):
        for sym in set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", text)):
            assert hasattr(lib, sym), sym
            proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S).group(1)
            nargs = 0 if proto.strip() in ("", "void") else proto.count(",") + 1
            assert set(call_arities(text, sym)) == {nargs}, sym


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
    for word in ("fr/mimc/mimc_mi355x.go", "SumBatchDevice", "NewDeviceTree", "gmsm_mimc_sum_batch", "gmsm_merkle_prove"):
        assert word in text, word
