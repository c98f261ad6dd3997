#!/usr/bin/env python3
"""Record what tests/test_params.py and tests/test_go_stubs.py check of the reference (gnark-crypto) into a small JSON
fixture, so that those tests need no reference tree: the field constants of fp/element.go and fr/element.go, the package
names, and the line numbers at which the definitions and calls the project cites sit (names and numbers only).

Output:  tests/golden/reference_facts.json
Run:     python tests/golden/make_reference_facts.py <gnark-crypto checkout>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = {"bn254": "bn254", "bls12_381": "bls12-381", "bw6_761": "bw6-761"}
TMPL = "internal/generator/ecc/template/multiexp.go.tmpl"

# file (relative to ecc/<curve>/ or to the checkout) -> [(label, text the line contains, label the search starts after)]
PER_CURVE = {
    "multiexp.go": [("G1Jac.MultiExp", "func (p *G1Jac) MultiExp(", None), ("G2Jac.MultiExp", "func (p *G2Jac) MultiExp(", None)],
    "kzg/kzg.go": [("Commit", "func Commit(p []fr.Element, pk ProvingKey, nbTasks ...int) (Digest, error)", None),
                   ("Commit: MultiExp over pk.G1", "res.MultiExp(pk.G1[:len(p)], p, config)", "Commit"),
                   ("Open", "func Open(", None), ("BatchOpenSinglePoint", "func BatchOpenSinglePoint(", None),
                   ("ErrInvalidPolynomialSize", "ErrInvalidPolynomialSize", None), ("ErrMinSRSSize", "ErrMinSRSSize", None)],
    "kzg/marshal.go": [("SRS.ReadDump", "func (srs *SRS) ReadDump(", None), ("ReadDump: unsafe.ReadSlice", "unsafe.ReadSlice", "SRS.ReadDump"),
                       ("ProvingKey.WriteTo", "func (pk *ProvingKey) WriteTo(", None),
                       ("WriteTo: encode pk.G1", "enc.Encode(pk.G1)", "ProvingKey.WriteTo"),
                       ("ProvingKey.ReadFrom", "func (pk *ProvingKey) ReadFrom(", None),
                       ("ReadFrom: decode pk.G1", "dec.Decode(&pk.G1)", "ProvingKey.ReadFrom"),
                       ("ProvingKey.UnsafeReadFrom", "func (pk *ProvingKey) UnsafeReadFrom(", None),
                       ("UnsafeReadFrom: NoSubgroupChecks", "NoSubgroupChecks()", "ProvingKey.UnsafeReadFrom")],
    "marshal.go": [("Decoder: unsafeComputeY with the subgroup check", "unsafeComputeY(dec.subGroupCheck)", None),
                   ("isCompressed", "func isCompressed(msb byte) bool", None)],
    "g1.go": [("BatchJacobianToAffineG1", "func BatchJacobianToAffineG1(points []G1Jac) []G1Affine", None)],
}
TEMPLATE = [("TJacobian.MultiExp", "func (p *{{ $.TJacobian }}) MultiExp(", None),
            ("MultiExp of the first half", "_p.MultiExp(points[:nbPoints/2]", "TJacobian.MultiExp"),
            ("MultiExp of the second half", "p.MultiExp(points[nbPoints/2:]", "MultiExp of the first half")]


def locate(path, entries):
    """label -> 1-based number of the first line containing the text (after the line of `after`); absent when not found."""
    lines = open(path).read().splitlines()
    found = {}
    for label, text, after in entries:
        start = found.get(after, 0) if after else 0
        hit = next((i + 1 for i in range(start, len(lines)) if text in lines[i]), None)
        if hit is not None:
            found[label] = hit
    return found


def element_constants(path, nlimbs):
    txt = open(path).read()
    rs = re.search(r"var rSquare = Element\{\s*((?:\d+,\s*)+)\}", txt).group(1)
    return {"q": [int(re.search(rf"\bq{i}\s*(?:uint64)?\s*=\s*(\d+)", txt).group(1)) for i in range(nlimbs)],
            "q_inv_neg": int(re.search(r"const qInvNeg\s*(?:uint64)?\s*=\s*(\d+)", txt).group(1)),
            "limbs": int(re.search(r"Limbs\s*=\s*(\d+)", txt).group(1)),
            "bits": int(re.search(r"Bits\s*=\s*(\d+)", txt).group(1)),
            "r_square": [int(x) for x in re.findall(r"\d+", rs)]}


def main(ref):
    data = {"_source": "gnark-crypto: ecc/<curve>/{fp,fr}/element.go, multiexp.go, marshal.go, g1.go, kzg/, and " + TMPL,
            "constants": {}, "package": {}, "lines": {}}
    for name, d in CURVES.items():
        nlimbs = {"fp": {"bn254": 4, "bls12_381": 6, "bw6_761": 12}[name], "fr": {"bn254": 4, "bls12_381": 4, "bw6_761": 6}[name]}
        data["constants"][name] = {fld: element_constants(os.path.join(ref, "ecc", d, fld, "element.go"), n) for fld, n in nlimbs.items()}
        for rel, entries in PER_CURVE.items():
            key = f"ecc/{d}/{rel}"
            data["lines"][key] = locate(os.path.join(ref, key), entries)
        head = open(os.path.join(ref, "ecc", d, "multiexp.go")).read().splitlines()[:12]
        data["package"][f"ecc/{d}/multiexp.go"] = next(m.group(1) for m in (re.match(r"^package (\w+)$", ln) for ln in head) if m)
    data["lines"][TMPL] = locate(os.path.join(ref, TMPL), TEMPLATE)
    with open(os.path.join(HERE, "reference_facts.json"), "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
