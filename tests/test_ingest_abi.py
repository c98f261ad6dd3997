"""The ingest, handle and device-list entries of include/gmsm.h without a device: every argument refusal returns its code
and its text before any device work, in the order the header promises (*bad_index is reset to -1 before any refusal but
the one about bad_index itself), the empty calls return GMSM_OK, and handles that name nothing are refused by every entry
that takes one."""
import ctypes
import re

import numpy as np

OK, DEVICE, ARG = 0, 3, 4  # GMSM_OK, GMSM_ERR_DEVICE, GMSM_ERR_ARG
ONE_OF_POINTS = "give exactly one of points (host) / d_points (device)"
SHARDED_TAG = 1 << 62
UNKNOWN = 1 << 40  # no process registers that many handles
PLAIN_UNKNOWN = (0, UNKNOWN)
SHARDED_UNKNOWN = (SHARDED_TAG, SHARDED_TAG | UNKNOWN)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Bad:
    """An int64_t bad_index that starts at 7, so that a reset to -1 shows."""

    def __init__(self):
        self.v = ctypes.c_int64(7)

    @property
    def ref(self):
        self.v.value = 7
        return ctypes.byref(self.v)

    @property
    def value(self):
        return self.v.value


def setup(gm):
    lib = gm._lib.load()
    err = lambda: lib.gmsm_last_error().decode()
    buf = np.zeros((4, 8), dtype=np.uint64)  # four BN254 G1 points, or their 256 raw bytes
    return lib, err, buf


def test_bases_register_refusals(gm):
    lib, err, buf = setup(gm)
    h = ctypes.c_uint64(0)
    reg = lib.gmsm_bases_register
    assert reg(99, None, None, 4, None) == ARG and err() == "unknown group id"  # the group comes first
    assert reg(-1, _p(buf), None, 4, ctypes.byref(h)) == ARG and err() == "unknown group id"
    assert reg(0, _p(buf), None, 4, None) == ARG and err() == "gmsm_bases_register: out_handle is null"
    assert reg(0, None, None, 4, None) == ARG and err() == "gmsm_bases_register: out_handle is null"  # ... before the pointer pair
    assert reg(0, None, None, 4, ctypes.byref(h)) == ARG and err() == "gmsm_bases_register: " + ONE_OF_POINTS
    assert reg(0, _p(buf), _p(buf), 4, ctypes.byref(h)) == ARG and err() == "gmsm_bases_register: " + ONE_OF_POINTS
    assert h.value == 0


def _decode_refusals(lib, err, buf, fn, name):
    """gmsm_points_from_raw / gmsm_points_from_compressed: (group, bytes, n, check, out_affine, d_out_affine, bad_index)"""
    bad = Bad()
    assert fn(99, None, 4, 1, None, None, None) == ARG and err() == "unknown group id"
    assert fn(6, _p(buf), 4, 1, _p(buf), None, bad.ref) == ARG and err() == "unknown group id" and bad.value == 7
    assert fn(0, _p(buf), 4, 1, _p(buf), None, None) == ARG and err() == f"{name}: bad_index is null"
    assert fn(0, None, 4, 1, None, None, None) == ARG and err() == f"{name}: bad_index is null"  # before the other pointers
    assert fn(0, None, 0, 1, None, None, None) == ARG and err() == f"{name}: bad_index is null"  # ... and before n == 0
    # *bad_index is -1 from here on, whatever is refused next
    assert fn(0, None, 4, 1, _p(buf), None, bad.ref) == ARG and err() == f"{name}: null argument" and bad.value == -1
    assert fn(0, _p(buf), 4, 1, None, None, bad.ref) == ARG and err() == f"{name}: null argument" and bad.value == -1
    for check in (0, 1, 2):
        assert fn(0, None, 0, check, None, None, bad.ref) == OK and bad.value == -1  # n == 0: no device, nothing touched
    assert fn(5, _p(buf), 0, 1, _p(buf), None, bad.ref) == OK and bad.value == -1


def test_points_from_raw_refusals(gm):
    lib, err, buf = setup(gm)
    _decode_refusals(lib, err, buf, lib.gmsm_points_from_raw, "gmsm_points_from_raw")


def test_points_from_compressed_refusals(gm):
    lib, err, buf = setup(gm)
    _decode_refusals(lib, err, buf, lib.gmsm_points_from_compressed, "gmsm_points_from_compressed")


def test_points_validate_refusals(gm):
    lib, err, buf = setup(gm)
    val, name, bad = lib.gmsm_points_validate, "gmsm_points_validate", Bad()
    assert val(99, None, None, 4, 1, None) == ARG and err() == "unknown group id"
    assert val(7, _p(buf), None, 4, 1, bad.ref) == ARG and err() == "unknown group id" and bad.value == 7
    assert val(0, _p(buf), None, 4, 1, None) == ARG and err() == f"{name}: bad_index is null"
    assert val(0, None, None, 4, 1, None) == ARG and err() == f"{name}: bad_index is null"  # before the pointer pair
    assert val(0, None, None, 4, 1, bad.ref) == ARG and err() == f"{name}: {ONE_OF_POINTS}" and bad.value == -1
    assert val(0, _p(buf), _p(buf), 4, 1, bad.ref) == ARG and err() == f"{name}: {ONE_OF_POINTS}" and bad.value == -1
    assert val(0, None, None, 4, 0, bad.ref) == ARG and err() == f"{name}: {ONE_OF_POINTS}"  # the pair before check <= 0
    assert val(0, None, None, 0, 1, bad.ref) == OK and bad.value == -1  # n == 0: the pair is not looked at
    assert val(0, _p(buf), _p(buf), 0, 2, bad.ref) == OK and bad.value == -1
    for check in (0, -1):  # nothing to check: no device
        assert val(0, _p(buf), None, 4, check, bad.ref) == OK and bad.value == -1
        assert val(3, None, _p(buf), 4, check, bad.ref) == OK and bad.value == -1


def _register_encoded_refusals(lib, err, buf, fn, name, arg):
    """gmsm_bases_register_raw / _compressed: (group, bytes, n, check, out_handle, bad_index)"""
    bad, h = Bad(), ctypes.c_uint64(0)
    assert fn(99, None, 4, 1, None, None) == ARG and err() == "unknown group id"
    assert fn(6, _p(buf), 4, 1, ctypes.byref(h), bad.ref) == ARG and err() == "unknown group id" and bad.value == 7
    # out_handle and bad_index are one check, and it comes before the reset
    assert fn(0, _p(buf), 4, 1, ctypes.byref(h), None) == ARG and err() == f"{name}: null argument"
    assert fn(0, _p(buf), 4, 1, None, bad.ref) == ARG and err() == f"{name}: null argument" and bad.value == 7
    assert fn(0, None, 4, 1, None, None) == ARG and err() == f"{name}: null argument"  # before the bytes
    assert fn(0, None, 4, 1, ctypes.byref(h), bad.ref) == ARG and err() == f"{name}: {arg} is null" and bad.value == -1
    assert h.value == 0


def test_bases_register_raw_refusals(gm):
    lib, err, buf = setup(gm)
    _register_encoded_refusals(lib, err, buf, lib.gmsm_bases_register_raw, "gmsm_bases_register_raw", "raw")


def test_bases_register_compressed_refusals(gm):
    lib, err, buf = setup(gm)
    _register_encoded_refusals(lib, err, buf, lib.gmsm_bases_register_compressed, "gmsm_bases_register_compressed", "comp")


def test_points_compress_refusals(gm):
    lib, err, buf = setup(gm)
    comp, text = lib.gmsm_points_compress, "gmsm_points_compress: " + ONE_OF_POINTS + ", and out_comp"
    assert comp(99, None, None, 4, None) == ARG and err() == "unknown group id"
    assert comp(0, None, None, 4, _p(buf)) == ARG and err() == text
    assert comp(0, _p(buf), _p(buf), 4, _p(buf)) == ARG and err() == text
    assert comp(0, _p(buf), None, 4, None) == ARG and err() == text
    assert comp(0, None, _p(buf), 4, None) == ARG and err() == text
    assert comp(0, None, None, 0, None) == OK  # n == 0: no device, nothing touched
    assert comp(4, _p(buf), _p(buf), 0, None) == OK


def test_handles_that_name_nothing(gm):
    lib, err, buf = setup(gm)
    for h in PLAIN_UNKNOWN + SHARDED_UNKNOWN:
        assert lib.gmsm_bases_release(h) == ARG and err() == "unknown bases handle"
        for c in (0, 8):
            assert lib.gmsm_bases_precompute(h, c) == ARG and err() == "unknown bases handle"
        assert lib.gmsm_multiexp_bases(h, _p(buf), 4, 0, _p(buf)) == ARG and err() == "unknown bases handle"
        assert lib.gmsm_bases_table_bits(h) == 0
        # an fft domain handle has no tag: the tagged values are just large numbers
        assert lib.gmsm_fft_domain_release(h) == ARG and err() == "unknown fft domain handle"
        assert lib.gmsm_fft(h, _p(buf), None, 4, 0, 0, 0, None) == ARG and err() == "unknown fft domain handle"
    for h in PLAIN_UNKNOWN:  # the explicit sharded entry says what it wants before it looks the handle up
        assert lib.gmsm_multiexp_bases_sharded(h, _p(buf), 4, 0, 0, _p(buf)) == ARG
        assert err() == "gmsm_multiexp_bases_sharded: not a handle of gmsm_bases_register_sharded"
    for h in SHARDED_UNKNOWN:
        for mode in (0, 1, 2):
            assert lib.gmsm_multiexp_bases_sharded(h, _p(buf), 4, 0, mode, _p(buf)) == ARG and err() == "unknown bases handle"
    assert lib.gmsm_multiexp_collect(0, _p(buf)) == ARG and err() == "unknown MultiExp ticket"


def test_set_devices_refuses_a_device_that_is_not_there(gm):
    lib, err, _ = setup(gm)
    n = lib.gmsm_device_count()
    before = (ctypes.c_int * 64)()
    nbefore = lib.gmsm_get_devices(before, 64)
    for lst in [[n], [n + 3]] + ([[0, n]] if n else []):  # 0 devices on a build machine, 8 on a node
        arr = (ctypes.c_int * len(lst))(*lst)
        assert lib.gmsm_set_devices(arr, len(lst)) == DEVICE
        m = re.fullmatch(r"gmsm_set_devices: device (\d+) does not exist \((\d+) visible\)", err())
        assert m and int(m.group(1)) == lst[-1] and int(m.group(2)) == n
    assert lib.gmsm_set_devices(None, 1) == ARG and err() == "gmsm_set_devices: devices is null"
    after = (ctypes.c_int * 64)()
    assert lib.gmsm_get_devices(after, 64) == nbefore and list(after) == list(before)  # a refused list changes nothing
