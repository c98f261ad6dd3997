"""The FRI entries of include/gmsm.h without a device: the seven symbols are exported, declared with the stated arity and bound; the
header, ABI_SYMBOLS and INTEGRATION's table name the same seven; every error the host can decide without a domain - a domain
exists only on a device - returns GMSM_ERR_ARG with its text before any device work, and nothing is written. The refusals that
need a live domain or oracle (a cardinality below 16, len > N, a fold past nbSteps, a step not built, a position outside its
layer) are in tests/test_gpu_fri.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITIES = {"gmsm_fri_commit": 6, "gmsm_fri_info": 4, "gmsm_fri_root": 3, "gmsm_fri_fold": 3, "gmsm_fri_layer": 4, "gmsm_fri_query": 7,
           "gmsm_fri_release": 1}
ARG = 4  # GMSM_ERR_ARG


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_are_exported_declared_and_bound(gm):
    lib = gm._lib.load()
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        decls = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for sym, arity in ARITIES.items():
        assert sym in gm._lib.ABI_SYMBOLS
        f = getattr(lib, sym)
        assert f.restype is ctypes.c_int
        proto = re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
        assert proto, sym
        assert len(f.argtypes) == proto.group(1).count(",") + 1 == arity, sym


def test_the_same_seven_entries_everywhere(gm):
    with open(os.path.join(ROOT, "include", "gmsm.h")) as f:
        decls = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    want = set(ARITIES)
    assert set(re.findall(r"^int (gmsm_fri_\w+)\s*\(", decls, re.M)) == want
    assert {s for s in gm._lib.ABI_SYMBOLS if s.startswith("gmsm_fri_")} == want
    assert set(re.findall(r"gmsm_fri_[a-z]+", integration)) == want
    for curve in ("bn254", "bls12-381", "bw6-761"):
        with open(os.path.join(ROOT, "integration", "go", curve, "fr", "fri", "fri_mi355x.go")) as f:
            assert set(re.findall(r"C\.(gmsm_fri_\w+)\(", f.read())) <= want


def test_argument_errors_need_no_device(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    a = np.full((16, 4), 7, dtype=np.uint64)
    out = np.full((16, 4), 9, dtype=np.uint64)
    handle = ctypes.c_uint64(77)
    for h in (0, 1 << 40):  # no domain can exist without a device: every handle is unknown
        assert lib.gmsm_fri_commit(h, _p(a), None, 16, None, ctypes.byref(handle)) == ARG and err() == "unknown fft domain handle"
        assert lib.gmsm_fri_commit(h, None, None, 16, None, ctypes.byref(handle)) == ARG and err() == "unknown fft domain handle"
    assert handle.value == 77
    card, steps, done = ctypes.c_uint64(1), ctypes.c_uint(2), ctypes.c_uint(3)
    pos = np.zeros(2, dtype=np.uint64)
    cnt = np.full(2, 9, dtype=np.uint32)
    for h in (0, 1, 1 << 40):
        assert lib.gmsm_fri_info(h, ctypes.byref(card), ctypes.byref(steps), ctypes.byref(done)) == ARG and err() == "unknown fri oracle handle"
        assert lib.gmsm_fri_root(h, 0, _p(out)) == ARG and err() == "unknown fri oracle handle"
        assert lib.gmsm_fri_fold(h, _p(a), _p(out)) == ARG and err() == "unknown fri oracle handle"
        assert lib.gmsm_fri_layer(h, 0, _p(out), None) == ARG and err() == "unknown fri oracle handle"
        assert lib.gmsm_fri_query(h, _p(pos), 2, _p(out), _p(out), _p(out), _p(cnt)) == ARG and err() == "unknown fri oracle handle"
        assert lib.gmsm_fri_query(h, _p(pos), 0, None, None, None, None) == ARG  # a stale handle is refused before count == 0 is looked at
        assert lib.gmsm_fri_release(h) == ARG and err() == "unknown fri oracle handle"
    assert (card.value, steps.value, done.value) == (1, 2, 3) and (out == 9).all() and (cnt == 9).all() and (a == 7).all()
