"""The big-int GKR model (tests/gkr_model.py) against the reference's own facts: its eight golden proofs over the three scalar
fields, its topological-sort tests, the closed form of the eq table, and a prove / verify round trip with a real hash."""
import hashlib
import importlib.util
import json
import os

import pytest

import gkr_model as M
from conftest import rng_for

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gkr_vectors.json")
CURVES = ["bn254", "bls12_381", "bw6_761"]


def field(gm, curve):
    c = gm.curves.CURVES[curve]
    return M.Field(c.r, c.fr_limbs * 8)


def vectors():
    with open(FIXTURE) as f:
        return json.load(f)


class ConstHash:
    """test_vector_utils.MessageCounter with step 0: every digest is the field element `val`"""

    def __init__(self, F, val):
        self.out = F.to_bytes(val)

    def update(self, b):
        pass

    def digest(self):
        return self.out


def vector_case(F, v):
    """circuit, full assignment, expected proof (ints mod p) of one fixture entry, as newTestCase builds them"""
    circuit = [(g, ins) for g, ins in v["circuit"]]
    s = M.Sorted(circuit)
    a, ins, outs = [None] * len(circuit), iter(v["input"]), iter(v["output"])
    expected_out = {}
    for w in s.order:
        if s.is_input(w):
            a[w] = [x % F.p for x in next(ins)]
        elif s.is_output(w):
            expected_out[w] = [x % F.p for x in next(outs)]
    full = M.complete(circuit, a, F.p)
    proof = [{"partialSumPolys": [[x % F.p for x in poly] for poly in pw["partialSumPolys"]],
              "finalEvalProof": [x % F.p for x in (pw["finalEvalProof"] or [])]} for pw in v["proof"]]
    return circuit, full, expected_out, proof


@pytest.mark.parametrize("curve", CURVES)
def test_model_reproduces_the_reference_vectors(gm, curve):
    F = field(gm, curve)
    vs = vectors()
    assert len(vs) == 8
    for name, v in vs.items():
        assert v["hash"] == {"type": "const", "val": -1}
        circuit, full, expected_out, proof = vector_case(F, v)
        for w, out in expected_out.items():
            assert full[w] == out, name
        factory = lambda: ConstHash(F, v["hash"]["val"])
        assert M.prove(F, circuit, full, factory) == proof, name
        assert M.verify(F, circuit, full, proof, factory) is None, name
        assert M.verify(F, circuit, full, proof, lambda: ConstHash(F, 2)) is not None, name


@pytest.mark.parametrize("curve", CURVES)
def test_eq_loop_is_the_closed_form(gm, curve):
    F = field(gm, curve)
    rng = rng_for(0x6B72, CURVES.index(curve))
    for n in range(7):
        for special in (False, True):
            q = [int.from_bytes(rng.bytes(48), "big") % F.p for _ in range(n)]
            if special and n:
                q[0] = 0
                q[-1] = 1 if n > 1 else q[-1]
            scale = int.from_bytes(rng.bytes(48), "big") % F.p
            assert M.eq_loop([scale] + [0] * ((1 << n) - 1), q, F.p) == M.eq_closed(q, scale, F.p)
            if n:  # the table is eq(q, .): its entry at a boolean h is EvalEq(q, h)
                h = int(rng.integers(0, 1 << n))
                bits = [(h >> (n - 1 - i)) & 1 for i in range(n)]
                assert M.eq_closed(q, 1, F.p)[h] == M.eval_eq(q, bits, F.p)


def random_circuit_case(F, rng, nvars):
    """three wires: two inputs and a mul gate over them"""
    circuit = [(None, []), (None, []), ("mul", [0, 1])]
    n = 1 << nvars
    a = [[int.from_bytes(rng.bytes(48), "big") % F.p for _ in range(n)] for _ in range(2)] + [None]
    return circuit, M.complete(circuit, a, F.p)


@pytest.mark.parametrize("curve", CURVES)
def test_verify_accepts_its_proofs_and_rejects_tampering(gm, curve):
    F = field(gm, curve)
    rng = rng_for(0x6B73, CURVES.index(curve))
    circuit, full = random_circuit_case(F, rng, 3)
    proof = M.prove(F, circuit, full, hashlib.sha256)
    assert M.verify(F, circuit, full, proof, hashlib.sha256) is None
    bad = json.loads(json.dumps(proof))
    bad[2]["partialSumPolys"][1][0] = (bad[2]["partialSumPolys"][1][0] + 1) % F.p
    assert M.verify(F, circuit, full, bad, hashlib.sha256) is not None
    bad = json.loads(json.dumps(proof))
    bad[2]["finalEvalProof"][1] = (bad[2]["finalEvalProof"][1] + 1) % F.p
    assert M.verify(F, circuit, full, bad, hashlib.sha256) is not None
    wrong = list(full)
    wrong[2] = list(full[2])
    wrong[2][5] = (wrong[2][5] + 1) % F.p
    assert M.verify(F, circuit, wrong, proof, hashlib.sha256) is not None


def test_topological_sort_matches_the_reference():
    # TestTopSortTrivial, TestTopSortDeep, TestTopSortWide (gkr_test.go:477-511)
    assert M.Sorted([(None, [1]), (None, [])]).order == [1, 0]
    assert M.Sorted([(None, [2]), (None, [3]), (None, []), (None, [0])]).order == [2, 0, 3, 1]
    wide = [[3, 8], [6], [4], [], [], [9], [9], [9, 5, 2], [4, 3], []]
    assert M.Sorted([(None, ins) for ins in wide]).order == [3, 4, 2, 8, 0, 9, 5, 6, 1, 7]


def test_challenge_names():
    s = M.Sorted([(None, []), ("identity", [0]), ("identity", [0])])  # wire 0 has two claims: a comb challenge
    assert M.challenge_names(s, 2) == ["fC.0", "fC.1", "w2.pSP.0", "w2.pSP.1", "w1.pSP.0", "w1.pSP.1", "w0.comb", "w0.pSP.0", "w0.pSP.1"]


def test_fixture_regenerates_identically():
    # a gnark-crypto checkout: named by the environment, or lying beside this repository
    ref = os.environ.get("GNARK_CRYPTO_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference"))
    if not os.path.isdir(os.path.join(ref, "internal", "generator", "gkr", "test_vectors")):
        pytest.skip("no reference tree")
    spec = importlib.util.spec_from_file_location("make_gkr_vectors", os.path.join(HERE, "golden", "make_gkr_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(FIXTURE) as f:
        assert f.read() == mod.render(mod.collect(ref))
