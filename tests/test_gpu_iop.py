"""fr.BatchInvert and the iop ratio polynomials on the device (gnark-crypto_amd/iop.py over gmsm_fr_batch_invert,
gmsm_iop_ratio_copy_constraint, gmsm_iop_ratio_shuffled), every output limb for limb against the big-int model of
tests/iop_model.py (the loops of ratios.go and BatchInvert, literally), for the three scalar fields:
  - BatchInvert at lengths around a lane, a tile and several tiles, zeros at the first, the last, a lane-boundary and a
    tile-boundary position, an all-zero vector, host and device pointers, aliased and not
  - the copy constraint (m = 3, mixed layouts) at n = 1, 2, 4, 256, 512 with default lanes, and with forced lanes
    (GMSM_OPT_POLY_LANE_BITS) at 512 (two tiles), 2^17 (512 tiles: the carry pass spans two tiles of lanes) and, lanes of 4,
    2^12; a random permutation, and the identity (Z = 1 everywhere)
  - a zero denominator on a lane boundary and on a tile boundary: Z is 0 from the next index on, bit-exact before
  - the shuffled vectors (m = 2) at three of those shapes
  - all six expected forms against the model's Lagrange / Regular vector pushed through the package's fft.Domain / BitReverse
    in the order of ratios.go:248-273
  - the wrapper's ToLagrange of Canonical / Regular and LagrangeCoset / BitReverse inputs
  - device pointers made on a torch stream, inputs unchanged, the range error of a permutation value, four threads on one
    domain handle"""
import ctypes
import threading

import numpy as np
import pytest

import iop_model as M
from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
REG, REV = M.REGULAR, M.BIT_REVERSE
LAYOUTS3 = [REG, REV, REG]
# (poly_lane_bits, n): 0 = lanes by length (8 elements below 2^14: a tile is 2048)
COPY_SHAPES = [(0, 1), (0, 2), (0, 4), (0, 256), (0, 512), (1, 512), (1, 1 << 17), (3, 1 << 12)]
SHUFFLED_SHAPES = [(0, 4), (1, 512), (3, 1 << 12)]

_COPY, _SHUF = {}, {}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rand_limbs(c, rng, count):
    return random_field_limbs(rng, c.r, c.fr_limbs, count)


def copy_case(gm, curve, n):
    """entries (3 n limbs, layouts LAYOUTS3), a random permutation, beta, gamma and the model's Z, made once per (curve, n)"""
    if (curve, n) not in _COPY:
        c = gm.CURVES[curve]
        rng = rng_for(0x10B0, CURVES.index(curve), n)
        flat = rand_limbs(c, rng, 3 * n)
        flat.setflags(write=False)
        bg = rand_limbs(c, rng, 2)
        perm = rng.permutation(3 * n).astype(np.int64)
        vals = M.from_limbs(c, flat)
        beta, gamma = M.from_limbs(c, bg)
        entries = [(vals[j * n:(j + 1) * n], LAYOUTS3[j]) for j in range(3)]
        z = M.build_ratio_copy_constraint(c, entries, perm.tolist(), beta, gamma)
        _COPY[(curve, n)] = dict(flat=flat, entries=entries, perm=perm, bg=bg, beta=beta, gamma=gamma, z=M.to_limbs(c, z))
    return _COPY[(curve, n)]


def polys_of(flat, n, layouts, basis=2):
    return [(flat[j * n:(j + 1) * n], basis, layouts[j]) for j in range(len(layouts))]


FORM_LR = (2, REG)


@pytest.mark.parametrize("curve", CURVES)
def test_batch_invert_against_the_model(gm, curve):
    import torch
    c = gm.CURVES[curve]
    lib = gm._lib.load()
    gid = gm._lib.GROUP_IDS[(curve, "g1")]
    rng = rng_for(0x10B1, CURVES.index(curve))
    for n in (1, 2, 3, 255, 256, 257, 2049, (1 << 16) + 1):
        a = rand_limbs(c, rng, n)
        for k in (0, n - 1, 16, 2048, 4096):  # first, last, a lane boundary (lanes of 8 and of 16), tile boundaries
            if k < n:
                a[k] = 0
        exp = M.to_limbs(c, M.batch_invert(M.from_limbs(c, a), c.r))
        keep = a.copy()
        assert (gm.iop.BatchInvert(curve, a) == exp).all(), n
        assert (a == keep).all()
        al = a.copy()  # host, aliased
        assert lib.gmsm_fr_batch_invert(gid, _p(al), None, n, None, _p(al), None) == 0
        assert (al == exp).all(), n
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d = torch.from_numpy(a.view(np.int64).copy()).cuda() * 1  # produced by a kernel on s
            out = torch.empty_like(d)
            gm.iop.batch_invert_device(curve, d.data_ptr(), n, out.data_ptr(), s.cuda_stream)
            assert (d.cpu().numpy().view(np.uint64) == a).all()
            gm.iop.batch_invert_device(curve, d.data_ptr(), n, d.data_ptr(), s.cuda_stream)  # device, aliased
        s.synchronize()
        assert (out.cpu().numpy().view(np.uint64) == exp).all(), n
        assert (d.cpu().numpy().view(np.uint64) == exp).all(), n
    z = np.zeros((257, c.fr_limbs), dtype=np.uint64)
    assert (gm.iop.BatchInvert(curve, z) == 0).all()
    assert gm.iop.BatchInvert(curve, z[:0]).shape == (0, c.fr_limbs)


@pytest.mark.parametrize("lanes,n", COPY_SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_copy_constraint_against_the_model(gm, forced_options, curve, lanes, n):
    c = gm.CURVES[curve]
    case = copy_case(gm, curve, n)
    forced_options(poly_lane_bits=lanes)
    d = gm.fft.NewDomain(curve, n)
    try:
        z = gm.iop.BuildRatioCopyConstraint(curve, polys_of(case["flat"], n, LAYOUTS3), case["perm"], case["bg"][0], case["bg"][1], FORM_LR, d)
        assert z.shape == (n, c.fr_limbs) and (z == case["z"]).all()
        ident = np.arange(3 * n, dtype=np.int64)
        z1 = gm.iop.BuildRatioCopyConstraint(curve, polys_of(case["flat"], n, LAYOUTS3), ident, case["bg"][0], case["bg"][1], FORM_LR, d)
        assert (z1 == M.to_limbs(c, [1])[0]).all()
    finally:
        d.release()


@pytest.mark.parametrize("k", [7, 8, 2047, 2048])
@pytest.mark.parametrize("curve", CURVES)
def test_zero_denominator(gm, curve, k):
    """n = 4096, lanes of 8, tiles of 2048: d_k sits at position k + 1 of the denominator vector - the last element of a lane
    (k = 7) or of a tile (k = 2047), the first of the next (k = 8, 2048)"""
    c = gm.CURVES[curve]
    n, j = 4096, 2
    assert gm.get_option("poly_lane_bits") == 0 and LAYOUTS3[j] == REG
    case = copy_case(gm, curve, n)
    supp_q = int(case["perm"][k + j * n])
    w, g = M.generator(c, n), c.fr_mult_gen
    s = pow(g, supp_q // n, c.r) * pow(w, supp_q % n, c.r) % c.r
    entries = [(list(v), l) for v, l in case["entries"]]
    entries[j][0][k] = (-case["beta"] * s - case["gamma"]) % c.r
    zm = M.build_ratio_copy_constraint(c, entries, case["perm"].tolist(), case["beta"], case["gamma"])
    assert zm[k + 1:] == [0] * (n - k - 1) and all(zm[:k + 1])
    flat = case["flat"].copy()
    flat[j * n + k] = M.to_limbs(c, [entries[j][0][k]])[0]
    z = gm.iop.BuildRatioCopyConstraint(curve, polys_of(flat, n, LAYOUTS3), case["perm"], case["bg"][0], case["bg"][1], FORM_LR)
    assert (z == M.to_limbs(c, zm)).all()
    assert (z[k + 1:] == 0).all() and (z[:k + 1] == case["z"][:k + 1]).all()


def shuffled_case(gm, curve, n):
    if (curve, n) not in _SHUF:
        c = gm.CURVES[curve]
        rng = rng_for(0x10B2, CURVES.index(curve), n)
        num, den = rand_limbs(c, rng, 2 * n), rand_limbs(c, rng, 2 * n)
        beta = rand_limbs(c, rng, 1)
        nl, dl = [REV, REG], [REG, REV]
        nv, dv = M.from_limbs(c, num), M.from_limbs(c, den)
        z = M.build_ratio_shuffled_vectors(c, [(nv[j * n:(j + 1) * n], nl[j]) for j in range(2)],
                                           [(dv[j * n:(j + 1) * n], dl[j]) for j in range(2)], M.from_limbs(c, beta)[0])
        _SHUF[(curve, n)] = dict(num=num, den=den, beta=beta[0], nl=nl, dl=dl, z=M.to_limbs(c, z))
    return _SHUF[(curve, n)]


@pytest.mark.parametrize("lanes,n", SHUFFLED_SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_shuffled_vectors_against_the_model(gm, forced_options, curve, lanes, n):
    case = shuffled_case(gm, curve, n)
    forced_options(poly_lane_bits=lanes)
    keep = case["num"].copy(), case["den"].copy()
    z = gm.iop.BuildRatioShuffledVectors(curve, polys_of(case["num"], n, case["nl"]), polys_of(case["den"], n, case["dl"]), case["beta"], FORM_LR)
    assert (z == case["z"]).all()
    assert (case["num"] == keep[0]).all() and (case["den"] == keep[1]).all()


@pytest.mark.parametrize("curve", CURVES)
def test_all_six_expected_forms(gm, forced_options, curve):
    """the model's Lagrange / Regular vector through putInExpectedFormFromLagrangeRegular (ratios.go:248-273) with the package's
    own transforms (pinned to the oracle by tests/test_gpu_fft.py), n = 512 with lanes of one element"""
    n = 512
    case = copy_case(gm, curve, n)
    forced_options(poly_lane_bits=1)
    fft = gm.fft
    d = fft.NewDomain(curve, n)
    try:
        for basis in (1, 2, 4):
            for layout in (REG, REV):
                exp = case["z"].copy()
                if basis == 1:
                    exp = d.FFTInverse(exp, fft.DIF)
                    if layout == REG:
                        exp = fft.BitReverse(curve, exp)
                elif basis == 4:
                    exp = d.FFT(d.FFTInverse(exp, fft.DIF), fft.DIT, fft.OnCoset())
                    if layout == REV:
                        exp = fft.BitReverse(curve, exp)
                elif layout == REV:
                    exp = fft.BitReverse(curve, exp)
                z = gm.iop.BuildRatioCopyConstraint(curve, polys_of(case["flat"], n, LAYOUTS3), case["perm"], case["bg"][0], case["bg"][1],
                                                    gm.iop.Form(basis, layout), d)
                assert (z == exp).all(), (basis, layout)
        sc = shuffled_case(gm, curve, n)
        z = gm.iop.BuildRatioShuffledVectors(curve, polys_of(sc["num"], n, sc["nl"]), polys_of(sc["den"], n, sc["dl"]), sc["beta"],
                                             gm.iop.Form(gm.iop.Canonical, gm.iop.Regular), d)
        assert (z == fft.BitReverse(curve, d.FFTInverse(sc["z"].copy(), fft.DIF))).all()
    finally:
        d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_wrapper_converts_its_inputs_to_lagrange(gm, curve):
    """the same entries given as Canonical / Regular and as LagrangeCoset / BitReverse yield the same Z (polynomial.go:296-315)"""
    n = 256
    case = copy_case(gm, curve, n)
    fft = gm.fft
    d = fft.NewDomain(curve, n)
    try:
        lag = [case["flat"][j * n:(j + 1) * n] for j in range(3)]
        lag = [fft.BitReverse(curve, v) if LAYOUTS3[j] == REV else v for j, v in enumerate(lag)]  # Lagrange / Regular
        canon = [fft.BitReverse(curve, d.FFTInverse(v, fft.DIF)) for v in lag]                     # Canonical / Regular
        coset = [d.FFT(v, fft.DIF, fft.OnCoset()) for v in canon]                                  # LagrangeCoset / BitReverse
        keep = [v.copy() for v in canon + coset]
        args = (case["perm"], case["bg"][0], case["bg"][1], FORM_LR)
        # the entries in Regular layout where the case has them bit-reversed: the same polynomials, so the same Z
        assert (gm.iop.BuildRatioCopyConstraint(curve, [(v, 1, REG) for v in canon], *args) == case["z"]).all()
        assert (gm.iop.BuildRatioCopyConstraint(curve, [(v, 4, REV) for v in coset], *args, d) == case["z"]).all()
        assert (gm.iop.BuildRatioCopyConstraint(curve, [(canon[0], 1, REG), (coset[1], 4, REV), (lag[2], 2, REG)], *args, d) == case["z"]).all()
        assert all((a == b).all() for a, b in zip(keep, canon + coset))  # inputs unchanged
    finally:
        d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointers_on_a_torch_stream(gm, curve):
    import torch
    c = gm.CURVES[curve]
    n = 512
    case, sc = copy_case(gm, curve, n), shuffled_case(gm, curve, n)
    d = gm.fft.NewDomain(curve, n)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda() * 1  # produced by a kernel on s
            ent, perm, num, den = up(case["flat"]), up(case["perm"]), up(sc["num"]), up(sc["den"])
            out = torch.empty(n * c.fr_limbs, dtype=torch.int64, device="cuda")
            out2 = torch.empty_like(out)
            gm.iop.build_ratio_copy_constraint_device(d, ent.data_ptr(), LAYOUTS3, perm.data_ptr(), case["bg"][0], case["bg"][1], FORM_LR,
                                                      out.data_ptr(), s.cuda_stream)
            gm.iop.build_ratio_shuffled_vectors_device(d, num.data_ptr(), sc["nl"], den.data_ptr(), sc["dl"], sc["beta"], FORM_LR,
                                                       out2.data_ptr(), s.cuda_stream)
        s.synchronize()
        host = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs)
        assert (host(out) == case["z"]).all() and (host(out2) == sc["z"]).all()
        assert (host(ent) == case["flat"]).all() and (perm.cpu().numpy() == case["perm"]).all()  # inputs unchanged
        assert (host(num) == sc["num"]).all() and (host(den) == sc["den"]).all()
    finally:
        d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_permutation_value_out_of_range(gm, curve):
    """perm[i] = m n: valid memory, a value the reference would index S with and panic. From the host and from the device."""
    import torch
    c = gm.CURVES[curve]
    n = 256
    case = copy_case(gm, curve, n)
    bad = case["perm"].copy()
    bad[300], bad[700] = 3 * n, -1
    msg = r"permutation\[300\] = 768 is outside \[0, 768\)"
    d = gm.fft.NewDomain(curve, n)
    try:
        with pytest.raises(ValueError, match=msg):
            gm.iop.BuildRatioCopyConstraint(curve, polys_of(case["flat"], n, LAYOUTS3), bad, case["bg"][0], case["bg"][1], FORM_LR, d)
        ent = torch.from_numpy(case["flat"].view(np.int64).copy()).cuda()
        perm = torch.from_numpy(bad).cuda()
        out = torch.zeros(n * c.fr_limbs, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match=msg):
            gm.iop.build_ratio_copy_constraint_device(d, ent.data_ptr(), LAYOUTS3, perm.data_ptr(), case["bg"][0], case["bg"][1], FORM_LR,
                                                      out.data_ptr())
        assert (out.cpu().numpy() == 0).all()  # nothing was written
        # the same permutation on the device with the result asked for on the host, bad and good
        lib = gm._lib.load()
        lay = np.array(LAYOUTS3, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        hout = np.zeros((n, c.fr_limbs), dtype=np.uint64)
        call = lambda pm: lib.gmsm_iop_ratio_copy_constraint(d.handle, None, ent.data_ptr(), 3, lay, None, pm.data_ptr(), _p(case["bg"][0]),
                                                             _p(case["bg"][1]), 2, REG, None, _p(hout), None)
        assert call(perm) == 4 and "permutation[300] = 768 is outside [0, 768)" in lib.gmsm_last_error().decode()
        assert (hout == 0).all()
        good = torch.from_numpy(case["perm"]).cuda()
        torch.cuda.synchronize()
        assert call(good) == 0 and (hout == case["z"]).all()
    finally:
        d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_output_overlapping_an_input_is_refused(gm, curve):
    """exact aliasing and an overlap of one element (host) or of a few bytes' worth (device), for every input vector"""
    import torch
    c = gm.CURVES[curve]
    n, nl = 256, c.fr_limbs
    lib = gm._lib.load()
    case = copy_case(gm, curve, n)
    u32 = lambda v: np.array(v, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    lay3, lay2 = u32(LAYOUTS3), u32([REG, REV])
    beta, gamma = case["bg"][0].copy(), case["bg"][1].copy()
    perm = case["perm"].copy()
    d = gm.fft.NewDomain(curve, n)
    try:
        def refused(rc):
            return rc == 4 and lib.gmsm_last_error().decode().endswith("the output overlaps an input (inputs are never modified)")
        big = np.zeros((4 * n, nl), dtype=np.uint64)
        big[:3 * n] = case["flat"]
        for out in (big[:n], big[2 * n:3 * n], big[3 * n - 1:4 * n - 1]):
            assert refused(lib.gmsm_iop_ratio_copy_constraint(d.handle, _p(big), None, 3, lay3, _p(perm), None, _p(beta), _p(gamma), 2, REG, None,
                                                              _p(out), None))
        assert (big[:3 * n] == case["flat"]).all() and (big[3 * n:] == 0).all()
        ok = big[3 * n:]  # adjacent, not overlapping
        assert lib.gmsm_iop_ratio_copy_constraint(d.handle, _p(big), None, 3, lay3, _p(perm), None, _p(beta), _p(gamma), 2, REG, None, _p(ok), None) == 0
        assert (ok == case["z"]).all()
        pbuf = np.zeros(3 * n + n * nl, dtype=np.int64)  # the permutation, then room for an output behind it
        pbuf[:3 * n] = perm
        for off in (0, 3 * n - 2):
            out = pbuf[off:off + n * nl]
            assert refused(lib.gmsm_iop_ratio_copy_constraint(d.handle, _p(big), None, 3, lay3, _p(pbuf), None, _p(beta), _p(gamma), 2, REG, None,
                                                              _p(out), None))
        num = np.zeros((3 * n, nl), dtype=np.uint64)
        den = np.zeros((3 * n, nl), dtype=np.uint64)
        for a, b, out in ((num, den, num[n:2 * n]), (num, den, den[:n]), (num, den, num[2 * n - 1:3 * n - 1]), (num, den, den[2 * n - 1:3 * n - 1])):
            assert refused(lib.gmsm_iop_ratio_shuffled(d.handle, _p(a), None, _p(b), None, 2, lay2, lay2, _p(beta), 2, REG, None, _p(out), None))
        # on the device
        dev = torch.zeros(4 * n * nl, dtype=torch.int64, device="cuda")
        dperm = torch.zeros(3 * n + n * nl, dtype=torch.int64, device="cuda")
        other = torch.zeros(3 * n * nl, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for ptr in (dev.data_ptr(), dev.data_ptr() + (3 * n - 1) * nl * 8, dperm.data_ptr(), dperm.data_ptr() + (3 * n - 2) * 8):
            assert refused(lib.gmsm_iop_ratio_copy_constraint(d.handle, None, dev.data_ptr(), 3, lay3, None, dperm.data_ptr(), _p(beta), _p(gamma),
                                                              1, REG, None, None, ptr))
        for ptr in (dev.data_ptr() + n * nl * 8, other.data_ptr() + (2 * n - 1) * nl * 8):
            assert refused(lib.gmsm_iop_ratio_shuffled(d.handle, None, dev.data_ptr(), None, other.data_ptr(), 2, lay2, lay2, _p(beta), 4, REV, None,
                                                       None, ptr))
        assert (dev.cpu().numpy() == 0).all() and (other.cpu().numpy() == 0).all()
    finally:
        d.release()


@pytest.mark.parametrize("curve", CURVES)
def test_batch_invert_takes_the_g2_group_id(gm, curve):
    """the scalar field is the curve's: the G2 id gives the G1 id's bits"""
    c = gm.CURVES[curve]
    lib = gm._lib.load()
    a = rand_limbs(c, rng_for(0x10B3, CURVES.index(curve)), 300)
    a[0] = a[299] = 0
    exp = M.to_limbs(c, M.batch_invert(M.from_limbs(c, a), c.r))
    out = np.zeros_like(a)
    assert lib.gmsm_fr_batch_invert(gm._lib.GROUP_IDS[(curve, "g2")], _p(a), None, 300, None, _p(out), None) == 0
    assert (out == exp).all()


@pytest.mark.parametrize("curve", CURVES)
def test_four_threads_on_one_domain(gm, curve):
    n = 512
    case = copy_case(gm, curve, n)
    forms = [gm.iop.Form(b, l) for b, l in ((2, REG), (1, REG), (4, REV), (1, REV))]
    d = gm.fft.NewDomain(curve, n)
    try:
        run1 = lambda f: gm.iop.BuildRatioCopyConstraint(curve, polys_of(case["flat"], n, LAYOUTS3), case["perm"], case["bg"][0],
                                                         case["bg"][1], f, d)
        seq = [run1(f) for f in forms]
        got, errs = [None] * 4, []

        def run(i):
            try:
                for _ in range(3):
                    got[i] = run1(forms[i])
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs
        assert (seq[0] == case["z"]).all()
        for a, b in zip(seq, got):
            assert (a == b).all()
    finally:
        d.release()
