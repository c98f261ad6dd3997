"""The MultiLin and GKR claim entries of include/gmsm.h without a device: the seven symbols are exported, declared with the
stated arity and bound; the header's limits are the mirror's; every error the host can decide returns GMSM_ERR_ARG with its
text before any device work, and nothing is written; gate programs pass the checks of gmsm_iop_evaluate_expression with
their texts. fiatshamir.Transcript against its definition H(name || previous || bindings). And what can be checked of
integration/go/<curve>/gkr/gkr_*.go and iop/program_words.go without a Go toolchain: build tags, package, the same exported
functions in both builds, every C call declared and exported with the prototype's arity, three curves equal up to substitution."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITIES = {"gmsm_multilin_fold": 6, "gmsm_multilin_evaluate": 8, "gmsm_multilin_eq": 8, "gmsm_gkr_claim_new": 16,
           "gmsm_gkr_claim_next": 3, "gmsm_gkr_claim_final": 3, "gmsm_gkr_claim_release": 1}
ARG = 4  # GMSM_ERR_ARG
INPUT, CONST, POINT, ADD, SUB, MUL, NEG = 1, 2, 3, 4, 5, 6, 7


def header():
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        return f.read()


def test_symbols_are_exported_declared_and_bound(gm):
    lib = gm._lib.load()
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for sym, arity in ARITIES.items():
        assert sym in gm._lib.ABI_SYMBOLS
        f = getattr(lib, sym)
        assert f.restype is ctypes.c_int
        proto = re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
        assert proto, sym
        assert len(f.argtypes) == proto.group(1).count(",") + 1 == arity, sym


def test_header_limits_are_the_mirrors(gm):
    defs = {name: int(v) for name, v in re.findall(r"^#define GMSM_GKR_([A-Z_]+) (\d+)$", header(), re.M)}
    assert defs == {"MAX_INPUTS": gm.gkr.GKR_MAX_INPUTS, "MAX_DEGREE": gm.gkr.GKR_MAX_DEGREE} == {"MAX_INPUTS": 16, "MAX_DEGREE": 15}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ins(op, dst=0, a=0, b=0):
    return op | dst << 8 | a << 16 | b << 24


def test_multilin_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    a = np.full((8, 4), 7, dtype=np.uint64)
    r = np.ones((3, 4), dtype=np.uint64)
    out = np.full(4, 9, dtype=np.uint64)
    E = "gmsm_multilin_fold: "
    assert lib.gmsm_multilin_fold(99, _p(a), None, 8, _p(r), None) == ARG and "unknown group" in err()
    assert lib.gmsm_multilin_fold(0, _p(a), None, 0, _p(r), None) == ARG and err() == E + "len = 0 is not a power of two (a MultiLin has 2^n elements)"
    assert lib.gmsm_multilin_fold(0, _p(a), None, 6, _p(r), None) == ARG and err() == E + "len = 6 is not a power of two (a MultiLin has 2^n elements)"
    assert lib.gmsm_multilin_fold(0, _p(a), None, 1, _p(r), None) == ARG and err() == E + "len == 1: nothing to fold"
    assert lib.gmsm_multilin_fold(0, _p(a), None, 8, None, None) == ARG and err() == E + "r is null"
    assert lib.gmsm_multilin_fold(0, None, None, 8, _p(r), None) == ARG and E in err()
    assert lib.gmsm_multilin_fold(0, _p(a), 4096, 8, _p(r), None) == ARG and E in err()
    E = "gmsm_multilin_evaluate: "
    assert lib.gmsm_multilin_evaluate(99, _p(a), None, 8, _p(r), 3, None, _p(out)) == ARG and "unknown group" in err()
    assert lib.gmsm_multilin_evaluate(0, _p(a), None, 12, _p(r), 3, None, _p(out)) == ARG and "is not a power of two" in err()
    assert lib.gmsm_multilin_evaluate(0, _p(a), None, 8, _p(r), 4, None, _p(out)) == ARG and err() == E + "ncoords = 4 is more than log2 len = 3"
    assert lib.gmsm_multilin_evaluate(0, _p(a), None, 8, None, 3, None, _p(out)) == ARG and err() == E + "coords is null"
    assert lib.gmsm_multilin_evaluate(0, _p(a), None, 8, _p(r), 3, None, None) == ARG and err() == E + "out_value is null"
    assert lib.gmsm_multilin_evaluate(0, None, None, 8, _p(r), 3, None, _p(out)) == ARG and E in err()
    E = "gmsm_multilin_eq: "
    scale = np.ones(4, dtype=np.uint64)
    assert lib.gmsm_multilin_eq(99, _p(r), 3, _p(scale), 0, None, _p(a), None) == ARG and "unknown group" in err()
    for n in (64, 63, 60):
        assert lib.gmsm_multilin_eq(0, _p(r), n, _p(scale), 0, None, _p(a), None) == ARG
        assert err() == E + "n = %d: 2^n elements are beyond what size_t indexes" % n
    assert lib.gmsm_multilin_eq(0, None, 3, _p(scale), 0, None, _p(a), None) == ARG and err() == E + "q is null"
    assert lib.gmsm_multilin_eq(0, _p(r), 3, None, 0, None, _p(a), None) == ARG and err() == E + "scale is null"
    assert lib.gmsm_multilin_eq(0, _p(r), 3, _p(scale), 0, None, None, None) == ARG and E in err()
    assert lib.gmsm_multilin_eq(0, _p(a[5:]), 3, _p(scale), 0, None, _p(a), None) == ARG and err() == E + "out overlaps q"
    assert (a == 7).all() and (out == 9).all()


def test_claim_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    E = "gmsm_gkr_claim_new: "
    n = 8
    t0, t1 = np.full((n, 4), 3, dtype=np.uint64), np.full((n, 4), 5, dtype=np.uint64)
    consts = np.zeros((2, 4), dtype=np.uint64)
    points = np.ones((2, 3, 4), dtype=np.uint64)
    comb = np.ones(4, dtype=np.uint64)
    gj = np.full((16, 4), 9, dtype=np.uint64)
    handle = ctypes.c_uint64(77)
    good = [ins(INPUT, 0, 0), ins(INPUT, 1, 1), ins(MUL, 0, 0, 1)]

    def call(prog=good, group=0, n_consts=2, degree=2, tables=(t0, t1), d_tables=None, m=None, length=n, k=2, prog_len=None, null=()):
        words = np.array(prog if len(prog) else [0], dtype=np.uint32)
        m = (len(tables) if tables is not None else len(d_tables)) if m is None else m
        arr = lambda src: None if src is None else (ctypes.c_void_p * max(len(src), 1))(*[x if isinstance(x, int) or x is None else x.ctypes.data for x in src])
        keep = (arr(tables), arr(d_tables))
        return lib.gmsm_gkr_claim_new(
            group, None if "prog" in null else words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(prog) if prog_len is None else prog_len,
            None if "consts" in null else _p(consts), n_consts, degree, keep[0], keep[1], m, length, None if "points" in null else _p(points), k,
            None if "comb" in null else _p(comb), None, None if "gj" in null else _p(gj), None if "handle" in null else ctypes.byref(handle))

    assert call(group=99) == ARG and "unknown group" in err()
    assert call(length=0) == ARG and err() == E + "len = 0 is not a power of two (a MultiLin has 2^n elements)"
    assert call(length=12) == ARG and err() == E + "len = 12 is not a power of two (a MultiLin has 2^n elements)"
    assert call(length=1) == ARG and err() == E + "len == 1: a sumcheck needs at least one variable"
    assert call(m=0, tables=()) == ARG and err() == E + "need at least one input (m == 0)"
    assert call(m=17, tables=(t0,) * 17) == ARG and err() == E + "17 inputs, more than 16"
    assert call(degree=0) == ARG and err() == E + "degree = 0 is outside [1, 15]"
    assert call(degree=16) == ARG and err() == E + "degree = 16 is outside [1, 15]"
    assert call(k=0) == ARG and err() == E + "need at least one evaluation point (k == 0)"
    assert call(k=2, null=("comb",)) == ARG and err() == E + "comb is null with k >= 2"
    assert call(null=("prog",)) == ARG and err() == E + "prog is null"
    assert call(null=("consts",)) == ARG and err() == E + "consts is null"
    assert call(null=("points",)) == ARG and err() == E + "points is null"
    assert call(null=("gj",)) == ARG and err() == E + "out_gj and out_handle must not be null"
    assert call(null=("handle",)) == ARG and err() == E + "out_gj and out_handle must not be null"
    assert call(tables=None, d_tables=None, m=2) == ARG and E in err()
    assert call(tables=(t0, t1), d_tables=(4096, 8192)) == ARG and E in err()
    assert call(tables=(t0, None)) == ARG and err() == E + "tables[1] is null"
    assert call(tables=None, d_tables=(4096, None)) == ARG and err() == E + "d_tables[1] is null"
    # the program: the checks and texts of gmsm_iop_evaluate_expression
    assert call(prog=[]) == ARG and err() == E + "empty program"
    assert call(prog=good + [ins(POINT, 2)]) == ARG and err() == E + "instruction 3: POINT needs a domain (domain == 0)"
    assert call(prog=[ins(INPUT, 0, 0), ins(ADD, 1, 0, 1)]) == ARG and err() == E + "instruction 1: reads register 1 before any instruction wrote it"
    assert call(prog=good + [ins(INPUT, 2, 2)]) == ARG and err() == E + "instruction 3: input 2 of 2"
    assert call(prog=good + [ins(CONST, 2, 2)]) == ARG and err() == E + "instruction 3: constant 2 of 2"
    assert call(prog=good + [ins(9, 2, 0, 1)]) == ARG and err() == E + "instruction 3: unknown opcode 9"
    assert call(prog=[ins(INPUT, 16, 0)]) == ARG and err() == E + "instruction 0: register 16 is not below 16"
    # handles
    one = np.ones(4, dtype=np.uint64)
    for f in (lib.gmsm_gkr_claim_next, lib.gmsm_gkr_claim_final):
        assert f(0, _p(one), _p(gj)) == ARG and err() == "unknown gkr claim handle"
        assert f(1 << 40, _p(one), _p(gj)) == ARG and err() == "unknown gkr claim handle"
    assert lib.gmsm_gkr_claim_release(1 << 40) == ARG and err() == "unknown gkr claim handle"
    # nothing was written
    assert (gj == 9).all() and handle.value == 77 and (t0 == 3).all() and (t1 == 5).all()


def test_mirror_gates_trace_to_programs(gm):
    g = gm.gkr.Gates
    assert [g[k].Degree() for k in ("identity", "add", "sub", "neg", "mul")] == [1, 1, 1, 1, 2]
    assert list(g["identity"].code("bn254", 1).words) == [ins(INPUT, 0, 0)]
    assert list(g["mul"].code("bn254", 2).words) == [ins(INPUT, 0, 0), ins(INPUT, 1, 1), ins(MUL, 0, 0, 1)]
    assert [int(w) & 0xFF for w in g["add"].code("bn254", 3).words] == [INPUT, INPUT, ADD, INPUT, ADD]
    assert [int(w) & 0xFF for w in g["neg"].code("bn254", 1).words] == [INPUT, NEG]
    assert g["mul"].code("bn254", 2) is g["mul"].code("bn254", 2)  # traced once per input count


def test_mirror_topological_sort_and_challenge_names(gm):
    K = gm.gkr
    wide = [[3, 8], [6], [4], [], [], [9], [9], [9, 5, 2], [4, 3], []]  # TestTopSortWide (gkr_test.go:494-511)
    c = K.Circuit(K.Wire() for _ in wide)
    for w, inputs in zip(c, wide):
        w.Inputs = [c[j] for j in inputs]
    assert [c.index(w) for w in K.topological_sort(c)] == [3, 4, 2, 8, 0, 9, 5, 6, 1, 7]
    c = K.Circuit(K.Wire() for _ in range(3))
    c[1].Inputs, c[2].Inputs = [c[0]], [c[0]]
    c[1].Gate = c[2].Gate = K.Gates["identity"]
    names = K.ChallengeNames(K.topological_sort(c), 2, "p.")
    assert names == ["p.fC.0", "p.fC.1", "p.w2.pSP.0", "p.w2.pSP.1", "p.w1.pSP.0", "p.w1.pSP.1", "p.w0.comb", "p.w0.pSP.0", "p.w0.pSP.1"]


def test_transcript(gm):
    fs = gm.fiatshamir
    t = fs.NewTranscript(hashlib.sha256, "alpha", "beta")
    with pytest.raises(ValueError, match="^challenge not recorded in the transcript$"):
        t.Bind("gamma", b"x")
    with pytest.raises(ValueError, match="^challenge not recorded in the transcript$"):
        t.ComputeChallenge("gamma")
    with pytest.raises(ValueError, match="^the previous challenge is needed and has not been computed$"):
        t.ComputeChallenge("beta")
    t.Bind("alpha", b"one")
    t.Bind("alpha", b"two")
    t.Bind("beta", b"three")
    alpha = t.ComputeChallenge("alpha")
    assert alpha == hashlib.sha256(b"alpha" + b"one" + b"two").digest()
    with pytest.raises(ValueError, match="^challenge already computed, cannot be binded to other values$"):
        t.Bind("alpha", b"late")
    assert t.ComputeChallenge("beta") == hashlib.sha256(b"beta" + alpha + b"three").digest()
    assert t.ComputeChallenge("alpha") == alpha  # computed once


# ---- the Go files (integration/go/<curve>/gkr, and the accessor they need in integration/go/<curve>/iop), as far as they can be
# checked without a Go toolchain
GO = os.path.join(ROOT, "integration", "go")
GO_CURVES = {"bn254": ("ecc/bn254", "GMSM_BN254_"), "bls12-381": ("ecc/bls12-381", "GMSM_BLS12_381_"), "bw6-761": ("ecc/bw6-761", "GMSM_BW6_761_")}
GO_FILES = [("gkr", "gkr_mi355x.go"), ("gkr", "gkr_purego.go"), ("iop", "program_words.go")]
GO_EXPORTED = ["Emit"] * 5 + ["ProveDevice"]


def read_go(curve, package, name):
    with open(os.path.join(GO, curve, package, name)) as f:
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


@pytest.mark.parametrize("curve", sorted(GO_CURVES))
def test_go_files(gm, curve):
    path, ids = GO_CURVES[curve]
    dev, pure, words = (read_go(curve, p, n) for p, n in GO_FILES)
    assert dev.startswith("//go:build mi355x\n") and pure.startswith("//go:build !mi355x\n")  # file-level, mutually exclusive
    assert "//go:build" not in words and 'import "C"' not in words  # one file for both builds
    assert re.search(r"^package iop$", words, re.M) and "func (p *Program) Words(result Sym) ([]uint32, []fr.Element, error) {" in words
    # the exported API: functions, and methods of exported types (deviceClaims is the unexported sumcheck.Claims of the device build)
    api = lambda text: re.sub(r"^func \(c \*deviceClaims\) .*$", "", text, flags=re.M)
    exported = lambda text: re.findall(r"^func (?:\(\w* ?\*?\w+\) )?([A-Z]\w*)\(", api(text), re.M)
    sig = lambda text: re.findall(r"^func ((?:\(\w* ?\*?\w+\) )?[A-Z]\w*\(.*)\{$", api(text), re.M)
    for text in (dev, pure):
        assert re.search(r"^package gkr$", text, re.M)
        assert f'"github.com/consensys/gnark-crypto/{path}/fr/iop"' in text and '"github.com/consensys/gnark-crypto/fiat-shamir"' in text
        assert exported(text) == GO_EXPORTED  # the same exported functions and methods in both builds
        assert re.search(r"^type DeviceGate interface \{\n\tGate\n\tEmit\(p \*iop\.Program, in \[\]iop\.Sym\) iop\.Sym\n\}$", text, re.M)
        for gate in ("IdentityGate", "AddGate", "MulGate", "SubGate", "NegGate"):  # the five named gates implement it
            assert re.search(rf"^func \((?:g )?{gate}\) Emit\(p \*iop\.Program, in \[\]iop\.Sym\) iop\.Sym \{{$", text, re.M), gate
    assert sig(dev) == sig(pure) and len(sig(dev)) == len(GO_EXPORTED)  # ... with the same signatures
    assert sorted(re.findall(r"^func \(c \*deviceClaims\) ([A-Z]\w*)\(", dev, re.M)) == ["ClaimsNum", "Combine", "Next", "ProveFinalEval", "VarsNum"]  # sumcheck.Claims
    assert "func ProveDevice(c Circuit, assignment WireAssignment, transcriptSettings fiatshamir.Settings, options ...Option) (Proof, error) {" in dev
    assert 'import "C"' not in pure and "C." not in re.sub(r"//.*", "", pure)
    assert "return Prove(c, assignment, transcriptSettings, options...)" in pure  # the build without the tag goes through the reference's Prove
    for ref in ("wire.Gate.(DeviceGate)", "a gate of the circuit is no DeviceGate", "runtime.Pinner", "getFirstChallengeNames(", "claims.deleteClaim(wire)",
                f"C.{ids}G1"):
        assert ref in dev  # a gate without a device form is refused; the reference's flow stays in the wrapper
    called = set(re.findall(r"C\.(gmsm_[a-z0-9_]+)\(", dev))
    assert called == {"gmsm_gkr_claim_new", "gmsm_gkr_claim_next", "gmsm_gkr_claim_final", "gmsm_gkr_claim_release", "gmsm_last_error"}
    decls = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = gm._lib.load()
    for sym in called:
        assert hasattr(lib, sym)
        proto = re.search(rf"\b{sym}\s*\(([^;]*?)\)\s*;", decls, re.S)
        arity = 0 if proto.group(1).strip() == "void" else proto.group(1).count(",") + 1
        assert set(call_arities(dev, sym)) == {arity}, sym


@pytest.mark.parametrize("curve", sorted(GO_CURVES))
def test_three_curves_equal_up_to_substitution(curve):
    path, ids = GO_CURVES[curve]
    for package, name in GO_FILES:
        base = read_go("bn254", package, name).replace("ecc/bn254", path).replace("GMSM_BN254_", ids)
        assert base == read_go(curve, package, name), name
