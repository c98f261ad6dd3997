"""The fflonk entries of the C ABI without a GPU: exported, declared with the stated arity and bound in _lib.py, the Python
mirror gm.fflonk carries the documented names, NextDivisor through the ABI equals the model, and the argument errors that
need neither a device nor a registered handle return GMSM_ERR_ARG with their texts (the refusals that depend on the
scalar field of a registered handle - equal points, the size condition - are in tests/test_gpu_fflonk.py)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import fflonk_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gmsm_fflonk_next_divisor": 3, "gmsm_fflonk_fold": 8, "gmsm_fflonk_fold_commit": 8, "gmsm_fflonk_open_w": 15,
         "gmsm_fflonk_open_wprime": 15}
CURVES = ["bn254", "bls12_381", "bw6_761"]


def _proto(decls, sym):
    return re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)


def test_symbols_exported_and_declared(gm):
    lib = gm._lib.load()
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for sym, arity in ARITY.items():
        assert sym in gm._lib.ABI_SYMBOLS
        assert hasattr(lib, sym), sym
        proto = _proto(decls, sym)
        assert proto, sym
        assert proto.group(1).count(",") + 1 == arity, sym
        assert len(getattr(lib, sym).argtypes) == arity, sym
        assert sym in header.replace(proto.group(0), "")  # the documentation block names it too
    for word in ("pack_sizes", "npoints", "gamma", "hip_stream", "out_claimed", "out_folded_claimed", "out_w", "d_out_w", "out_w_jac"):
        assert word in _proto(decls, "gmsm_fflonk_open_w").group(1)
    for word in ("pack_sizes", "folded_claimed", "d_w", "z", "out_wprime_jac"):
        assert word in _proto(decls, "gmsm_fflonk_open_wprime").group(1)
    for word in ("d_out_folded", "out_jac"):
        assert word in _proto(decls, "gmsm_fflonk_fold_commit").group(1)
    # pointer against integer arguments, position by position
    for sym in ARITY:
        params = [p.strip() for p in _proto(decls, sym).group(1).split(",")]
        for param, argtype in zip(params, getattr(lib, sym).argtypes):
            is_pointer = "*" in param
            assert is_pointer == (argtype in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t))), (sym, param)


def test_python_mirror_names(gm):
    for name in ("NextDivisor", "Fold", "FoldAndCommit", "OpenW", "OpenWPrime", "BatchOpen", "fold_device", "open_w_device",
                 "open_wprime_device"):
        assert callable(getattr(gm.fflonk, name)), name
    # ErrNbPolynomialsNbPoints, fflonk.go:21
    assert gm.fflonk.ERR_NB_PACKS == "the number of packs of polynomials should be the same as the number of pack of points"


@pytest.mark.parametrize("curve", CURVES)
def test_next_divisor_through_the_abi(gm, curve):
    c = gm.CURVES[curve]
    assert [gm.fflonk.NextDivisor(curve, n) for n in range(1, 17)] == [fm.next_divisor(n, c.r) for n in range(1, 17)]
    L, t = gm._lib.load(), ctypes.c_size_t(0)
    for which in ("g1", "g2"):  # a property of the scalar field: both groups of a curve answer
        assert L.gmsm_fflonk_next_divisor(gm._lib.GROUP_IDS[(curve, which)], 5, ctypes.byref(t)) == 0 and t.value == 6
    # large sizes, the 100-trial limit and its edge (a divisor met as the counter reaches zero is refused, as the reference panics)
    d = next(t for t in itertools.count(1 << 20) if (c.r - 1) % t == 0 and all((c.r - 1) % u for u in range(t - 100, t)))
    assert gm.fflonk.NextDivisor(curve, d - 99) == d and gm.fflonk.NextDivisor(curve, d) == d
    for n in (d - 100, next(n for n in itertools.count(1 << 33) if fm.next_divisor(n, c.r) is None)):
        with pytest.raises(ValueError, match="did not find any divisor of r-1 within 100 trials"):
            gm.fflonk.NextDivisor(curve, n)
    big = 1  # a divisor of r - 1 above 2^40, from its small prime factors: a size beyond 32 bits
    rest = c.r - 1
    for q in range(2, 1000):
        while rest % q == 0 and big <= 1 << 40:
            big, rest = big * q, rest // q
    assert 1 << 40 < big < 1 << 63 and (c.r - 1) % big == 0
    got = gm.fflonk.NextDivisor(curve, big - 50)
    assert got == fm.next_divisor(big - 50, c.r) and big - 50 <= got <= big
    ARG = gm._lib.GMSM_ERR_ARG
    assert L.gmsm_fflonk_next_divisor(gm._lib.GROUP_IDS[(curve, "g1")], 0, ctypes.byref(t)) == ARG and "n == 0" in gm._lib.last_error()
    assert L.gmsm_fflonk_next_divisor(gm._lib.GROUP_IDS[(curve, "g1")], 4, None) == ARG
    assert L.gmsm_fflonk_next_divisor(99, 4, ctypes.byref(t)) == ARG and gm._lib.last_error() == "unknown group id"


def _u64(n):
    return np.zeros(n, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sizes(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_open_argument_errors_without_a_device(gm):
    L = gm._lib.load()
    ARG = gm._lib.GMSM_ERR_ARG
    polys, points, gamma, z, claimed, folded, w, jac = _u64(32), _u64(8), _u64(4), _u64(4), _u64(16), _u64(16), _u64(16), _u64(12)
    lens, sizes, npts = _sizes(4, 4), _sizes(1, 1), _sizes(1, 1)

    def open_w(handle=12345, polys_=_p(polys), d_polys=None, lens_=lens, sizes_=sizes, k=2, points_=_p(points), npts_=npts, gamma_=_p(gamma),
               claimed_=_p(claimed), folded_=_p(folded), w_=_p(w), d_w=None, jac_=_p(jac)):
        return L.gmsm_fflonk_open_w(handle, polys_, d_polys, lens_, sizes_, k, points_, npts_, gamma_, None, claimed_, folded_, w_, d_w, jac_)

    def open_wprime(handle=12345, polys_=_p(polys), d_polys=None, lens_=lens, sizes_=sizes, k=2, points_=_p(points), npts_=npts,
                    folded_=_p(folded), gamma_=_p(gamma), w_=_p(w), d_w=None, z_=_p(z), jac_=_p(jac)):
        return L.gmsm_fflonk_open_wprime(handle, polys_, d_polys, lens_, sizes_, k, points_, npts_, folded_, gamma_, w_, d_w, z_, None, jac_)

    for call in (open_w, open_wprime):
        assert call() == ARG and gm._lib.last_error() == "unknown bases handle"  # nothing is registered in this process
        assert call(k=0) == ARG and "no pack of polynomials" in gm._lib.last_error()
        assert call(lens_=None) == ARG and call(sizes_=None) == ARG and call(points_=None) == ARG and call(npts_=None) == ARG
        assert call(gamma_=None) == ARG and call(jac_=None) == ARG and call(folded_=None) == ARG
        assert call(polys_=None) == ARG and "exactly one of polys (host) / d_polys (device)" in gm._lib.last_error()
        assert call(d_polys=_p(polys)) == ARG and "exactly one of" in gm._lib.last_error()
    assert open_w(claimed_=None) == ARG and "out_claimed" in gm._lib.last_error()
    assert open_w(w_=None) == ARG and "exactly one of out_w (host) / d_out_w (device)" in gm._lib.last_error()
    assert open_w(d_w=_p(w)) == ARG and "exactly one of" in gm._lib.last_error()
    assert open_w(w_=_p(polys)) == ARG and "aliases" in gm._lib.last_error()
    assert open_w(folded_=_p(claimed)) == ARG and "aliases" in gm._lib.last_error()
    assert open_wprime(w_=None) == ARG and "exactly one of w (host) / d_w (device)" in gm._lib.last_error()
    assert open_wprime(d_w=_p(w)) == ARG and "exactly one of" in gm._lib.last_error()
    assert open_wprime(z_=None) == ARG
    assert open_wprime(jac_=_p(polys)) == ARG and "aliases" in gm._lib.last_error()


@pytest.mark.parametrize("curve", CURVES)
def test_fold_argument_errors_without_a_device(gm, curve):
    """gmsm_fflonk_fold takes a group, so its pack checks run here: they precede any device work"""
    L = gm._lib.load()
    ARG = gm._lib.GMSM_ERR_ARG
    c = gm.CURVES[curve]
    gid = gm._lib.GROUP_IDS[(curve, "g1")]
    polys, out, jac = _u64(8 * c.fr_limbs), _u64(64 * c.fr_limbs), _u64(3 * c.fp_limbs)

    def fold(group=gid, polys_=_p(polys), d_polys=None, lens_=_sizes(4, 4), n=2, out_=_p(out), d_out=None):
        return L.gmsm_fflonk_fold(group, polys_, d_polys, lens_, n, None, out_, d_out)

    assert fold(group=99) == ARG and gm._lib.last_error() == "unknown group id"
    assert fold(n=0) == ARG and "no polynomial" in gm._lib.last_error()
    assert fold(lens_=None) == ARG
    assert fold(polys_=None) == ARG and "exactly one of polys (host) / d_polys (device)" in gm._lib.last_error()
    assert fold(d_polys=_p(polys)) == ARG and "exactly one of" in gm._lib.last_error()
    assert fold(out_=None) == ARG and "exactly one of out (host) / d_out (device)" in gm._lib.last_error()
    assert fold(d_out=_p(out)) == ARG and "exactly one of" in gm._lib.last_error()
    assert fold(out_=_p(polys)) == ARG and "aliases" in gm._lib.last_error()
    assert fold(lens_=_sizes(0, 0)) == ARG and "polynomial 0 is empty (eval reads p[len(p)-1])" in gm._lib.last_error()
    n = next(n for n in itertools.count(1 << 20) if fm.next_divisor(n, c.r) is None)
    assert fold(lens_=(ctypes.c_size_t * n)(), n=n) == ARG and "did not find any divisor of r-1 within 100 trials" in gm._lib.last_error()
    # FoldAndCommit: the pointer checks, then the handle
    commit = lambda handle=12345, polys_=_p(polys), d_polys=None, lens_=_sizes(4, 4), n_=2, jac_=_p(jac): \
        L.gmsm_fflonk_fold_commit(handle, polys_, d_polys, lens_, n_, None, None, jac_)
    assert commit() == ARG and gm._lib.last_error() == "unknown bases handle"
    assert commit(jac_=None) == ARG and "out_jac is null" in gm._lib.last_error()
    assert commit(n_=0) == ARG and "no polynomial" in gm._lib.last_error()
    assert commit(polys_=None) == ARG and "exactly one of" in gm._lib.last_error()
    assert commit(jac_=_p(polys)) == ARG and "aliases" in gm._lib.last_error()


def test_python_mirror_raises_reference_error(gm):
    class FakeBases:
        handle = 12345
        group = gm.G1Affine("bn254")
    f, pt = np.zeros((3, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match="the number of packs of polynomials should be the same as the number of pack of points"):
        gm.fflonk.OpenW([[f], [f]], [pt], pt[0], FakeBases())
    with pytest.raises(ValueError, match="the number of packs of polynomials should be the same as the number of pack of points"):
        gm.fflonk.BatchOpen([[f]], [pt, pt], pt[0], lambda W: pt[0], FakeBases())
    with pytest.raises(ValueError, match="folded_claimed"):
        gm.fflonk.OpenWPrime([[f, f]], [pt], [np.zeros((3, 4), dtype=np.uint64)], pt[0], np.zeros((6, 4), dtype=np.uint64), pt[0], FakeBases())
    with pytest.raises(ValueError, match="w must have"):
        gm.fflonk.OpenWPrime([[f, f]], [pt], [np.zeros((2, 4), dtype=np.uint64)], pt[0], f, pt[0], FakeBases())
    with pytest.raises(ValueError, match="unknown bases handle"):
        gm.fflonk.OpenW([[f]], [pt], pt[0], FakeBases())
    with pytest.raises(ValueError, match="unknown bases handle"):
        gm.fflonk.FoldAndCommit([f], FakeBases())
