"""The shplonk entries of the C ABI without a GPU: exported, declared with the stated arity and bound in _lib.py, the
Python mirror gm.shplonk carries the documented names, and the argument errors that need neither a device nor a registered
handle return GMSM_ERR_ARG with their texts."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gmsm_shplonk_open_w": 13, "gmsm_shplonk_open_wprime": 14}


def test_symbols_exported_and_declared(gm):
    lib = gm._lib.load()
    header = open(os.path.join(ROOT, "include", "gmsm.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for sym, arity in ARITY.items():
        assert sym in gm._lib.ABI_SYMBOLS
        assert hasattr(lib, sym), sym
        proto = re.search(rf"^int {sym}\s*\(([^;]*?)\)\s*;", decls, re.S | re.M)
        assert proto, sym
        assert proto.group(1).count(",") + 1 == arity, sym
        assert len(getattr(lib, sym).argtypes) == arity, sym
        assert sym in header.replace(proto.group(0), "")  # the documentation block names it too
    for word in ("out_claimed", "out_w", "d_out_w", "out_w_jac", "npoints", "gamma", "hip_stream"):
        assert word in re.search(r"^int gmsm_shplonk_open_w\s*\(([^;]*?)\)\s*;", decls, re.S | re.M).group(1)
    for word in ("claimed", "d_w", "z", "out_wprime_jac"):
        assert word in re.search(r"^int gmsm_shplonk_open_wprime\s*\(([^;]*?)\)\s*;", decls, re.S | re.M).group(1)


def test_python_mirror_names(gm):
    for name in ("OpenW", "OpenWPrime", "open_w_device", "open_wprime_device", "BatchOpen"):
        assert callable(getattr(gm.shplonk, name)), name
    assert gm.shplonk.ERR_NB_POINTS == "number of digests should be equal to the number of points"  # ErrInvalidNumberOfPoints


def _u64(n):
    return np.zeros(n, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sizes(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_argument_errors_without_a_device(gm):
    L = gm._lib.load()
    ARG = gm._lib.GMSM_ERR_ARG
    polys, points, gamma, z, claimed, w, jac = _u64(32), _u64(8), _u64(4), _u64(4), _u64(8), _u64(16), _u64(12)
    lens, npts = _sizes(4, 4), _sizes(1, 1)

    def open_w(handle=12345, polys_=_p(polys), d_polys=None, lens_=lens, k=2, points_=_p(points), npts_=npts, gamma_=_p(gamma),
               claimed_=_p(claimed), w_=_p(w), d_w=None, jac_=_p(jac)):
        return L.gmsm_shplonk_open_w(handle, polys_, d_polys, lens_, k, points_, npts_, gamma_, None, claimed_, w_, d_w, jac_)

    def open_wprime(handle=12345, polys_=_p(polys), d_polys=None, lens_=lens, k=2, points_=_p(points), npts_=npts, claimed_=_p(claimed),
                    gamma_=_p(gamma), w_=_p(w), d_w=None, z_=_p(z), jac_=_p(jac)):
        return L.gmsm_shplonk_open_wprime(handle, polys_, d_polys, lens_, k, points_, npts_, claimed_, gamma_, w_, d_w, z_, None, jac_)

    for call in (open_w, open_wprime):
        assert call() == ARG and gm._lib.last_error() == "unknown bases handle"  # nothing is registered in this process
        assert call(k=0) == ARG and "no polynomial" in gm._lib.last_error()
        assert call(lens_=None) == ARG and call(points_=None) == ARG and call(npts_=None) == ARG and call(gamma_=None) == ARG
        assert call(jac_=None) == ARG and call(claimed_=None) == ARG
        assert call(polys_=None) == ARG and "exactly one of polys (host) / d_polys (device)" in gm._lib.last_error()
        assert call(d_polys=_p(polys)) == ARG and "exactly one of" in gm._lib.last_error()
    assert open_w(w_=None) == ARG and "exactly one of out_w (host) / d_out_w (device)" in gm._lib.last_error()
    assert open_w(d_w=_p(w)) == ARG and "exactly one of" in gm._lib.last_error()
    assert open_w(w_=_p(polys)) == ARG and "aliases" in gm._lib.last_error()
    assert open_wprime(w_=None) == ARG and "exactly one of w (host) / d_w (device)" in gm._lib.last_error()
    assert open_wprime(d_w=_p(w)) == ARG and "exactly one of" in gm._lib.last_error()
    assert open_wprime(z_=None) == ARG
    assert open_wprime(jac_=_p(polys)) == ARG and "aliases" in gm._lib.last_error()


def test_python_mirror_raises_reference_error(gm):
    class FakeBases:
        handle = 12345
        group = gm.G1Affine("bn254")
    f, pt = np.zeros((3, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match="number of digests should be equal to the number of points"):
        gm.shplonk.OpenW([f, f], [pt], pt[0], FakeBases())
    with pytest.raises(ValueError, match="number of digests should be equal to the number of points"):
        gm.shplonk.BatchOpen([f], [pt, pt], pt[0], lambda W: pt[0], FakeBases())
    with pytest.raises(ValueError, match="number of digests should be equal to the number of points"):
        gm.shplonk.OpenWPrime([f], [pt], [np.zeros((2, 4), dtype=np.uint64)], pt[0], f, pt[0], FakeBases())
    with pytest.raises(ValueError, match="unknown bases handle"):
        gm.shplonk.OpenW([f], [pt], pt[0], FakeBases())
