"""fr/fft on the device (gmsm_fft_*, gnark-crypto_amd/fft.py) against the oracle, bit for bit: every decimation,
direction and coset combination, sizes 1 .. 2^16 for the three scalar fields, 2^22 for BN254, plus the reference's
round-trip properties (ecc/bn254/fr/fft/fft_test.go) at a size the oracle does not need to touch; then the pass shapes the
size table of FftField::run selects between and above those sizes (2^15, 2^17 .. 2^19, 2^21, 2^22 for the other fields)."""
import numpy as np
import pytest

from conftest import random_field_limbs, rng_for

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "bls12_381", "bw6_761"]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_domain_constants(gm, oracle_mod, curve):
    F = oracle_mod.FFT(curve)
    c = F.curve
    fr = oracle_mod.Field(f"{c.name}_fr", c.fr_limbs)
    for m in (1, 5, 1 << 10, (1 << 16) + 1):
        d = gm.fft.NewDomain(curve, m)
        x = 1
        while x < m:
            x <<= 1
        assert d.Cardinality == x
        assert (d.Generator == F.generator(m)).all()
        assert (fr.mul(d.Generator, d.GeneratorInv) == fr.to_mont(np.array([1] + [0] * (c.fr_limbs - 1), dtype=np.uint64))).all()
        one = fr.to_mont(np.array([1] + [0] * (c.fr_limbs - 1), dtype=np.uint64))
        assert (fr.mul(d.FrMultiplicativeGen, d.FrMultiplicativeGenInv) == one).all()
        card = fr.to_mont(np.array([x] + [0] * (c.fr_limbs - 1), dtype=np.uint64))
        assert (fr.mul(card, d.CardinalityInv) == one).all()
        d.release()
    with pytest.raises(ValueError):
        gm.fft.NewDomain(curve, 1 << (c.fr_max_order + 1))


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("logn", [0, 1, 2, 5, 10, 11, 12, 13, 16, 20])
def test_fft_matches_oracle(gm, oracle_mod, curve, logn):
    F = oracle_mod.FFT(curve)
    c = F.curve
    n = 1 << logn
    a = random_field_limbs(rng_for(81, logn, c.fr_limbs), c.r, c.fr_limbs, n)
    d = gm.fft.NewDomain(curve, n)
    for inverse in (False, True):
        for dec in (gm.fft.DIT, gm.fft.DIF):
            for coset in (False, True):
                opts = (gm.fft.OnCoset(),) if coset else ()
                got = (d.FFTInverse if inverse else d.FFT)(a, dec, *opts)
                want = F.transform(a, inverse=inverse, decimation=dec, coset=coset)
                assert (got == want).all(), (inverse, dec, coset)
    assert (gm.fft.BitReverse(curve, a) == F.bit_reverse(a)).all()
    d.release()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_fft_class_edges(gm, oracle_mod, curve):
    """Inputs that push the lazy-limb butterflies to the edge of their value class: every element r - 1 (eleven
    additions in a row double the largest representable residue each time), all zero, alternating, a single spike."""
    F = oracle_mod.FFT(curve)
    c = F.curve
    for logn in (11, 14):
        n = 1 << logn
        rm1 = np.array([(c.r - 1 >> (64 * k)) & (2**64 - 1) for k in range(c.fr_limbs)], dtype=np.uint64)
        fr = oracle_mod.Field(f"{c.name}_fr", c.fr_limbs)
        top = np.tile(fr.to_mont(rm1), (n, 1))  # Montgomery form of r - 1
        raw = np.tile(rm1, (n, 1))              # the limbs r - 1 themselves: the largest canonical limb pattern
        alt = raw.copy()
        alt[1::2] = 0
        spike = np.zeros_like(raw)
        spike[n // 3] = rm1
        d = gm.fft.NewDomain(curve, n)
        for a in (top, raw, alt, spike, np.zeros_like(raw)):
            for inverse in (False, True):
                for dec in (gm.fft.DIT, gm.fft.DIF):
                    for coset in (False, True):
                        opts = (gm.fft.OnCoset(),) if coset else ()
                        got = (d.FFTInverse if inverse else d.FFT)(a, dec, *opts)
                        want = F.transform(a, inverse=inverse, decimation=dec, coset=coset)
                        assert (got == want).all(), (logn, inverse, dec, coset)
        d.release()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_fft_decimations_and_entries_agree(gm, oracle_mod, curve):
    """Two independent routes to the same vector (fft_test.go:100-158): DIF followed by BitReverse equals BitReverse followed
    by DIT - different kernels passes, twiddle orders and scalings - for every direction and coset choice; and the
    device-pointer entry equals the host-buffer entry.  (Round 3's version of this test set switches of A/B paths that no
    longer exist and compared the default path with itself.)"""
    import torch
    cc = oracle_mod.FFT(curve).curve
    n = 1 << 13
    a = random_field_limbs(rng_for(83, cc.fr_limbs), cc.r, cc.fr_limbs, n)
    d = gm.fft.NewDomain(curve, n)
    stream = torch.cuda.current_stream().cuda_stream
    for inverse in (False, True):
        for coset in (False, True):
            opts = (gm.fft.OnCoset(),) if coset else ()
            run = d.FFTInverse if inverse else d.FFT
            via_dif = gm.fft.BitReverse(curve, run(a, gm.fft.DIF, *opts))
            via_dit = run(gm.fft.BitReverse(curve, a), gm.fft.DIT, *opts)
            assert (via_dif == via_dit).all(), (inverse, coset)
            t = torch.from_numpy(a.view(np.int64).copy()).cuda()
            d.fft_device(t.data_ptr(), gm.fft.DIF, *opts, inverse=inverse, stream=stream)
            gm.fft.BitReverse(curve, d_a=t.data_ptr(), n=n, stream=stream)
            assert (t.cpu().numpy().view(np.uint64) == via_dif).all(), (inverse, coset, "device entry")
    d.release()


@pytest.mark.parametrize("curve", ["bn254", "bw6_761"])
def test_first_coset_transform_from_two_threads(gm, oracle_mod, curve):
    """The coset tables of a domain appear with its FIRST coset transform; two threads that both make that first call must
    both get complete tables (the ready flag is set only after the build stream has been synchronised, gmsm_fft.h) - and
    a forward and an inverse caller race on different tables of the same domain."""
    import threading
    F = oracle_mod.FFT(curve)
    c = F.curve
    n = 1 << 14
    a = random_field_limbs(rng_for(84, c.fr_limbs), c.r, c.fr_limbs, n)
    want_f = F.transform(a, inverse=False, decimation=gm.fft.DIF, coset=True)
    want_i = F.transform(a, inverse=True, decimation=gm.fft.DIT, coset=True)
    for attempt in range(4):  # a fresh domain every time: the race is on the first use
        d = gm.fft.NewDomain(curve, n)
        res = [None] * 4
        start = threading.Barrier(4)

        def worker(k):
            start.wait()
            res[k] = d.FFT(a, gm.fft.DIF, gm.fft.OnCoset()) if k % 2 == 0 else d.FFTInverse(a, gm.fft.DIT, gm.fft.OnCoset())
        th = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for k in range(4):
            assert (res[k] == (want_f if k % 2 == 0 else want_i)).all(), (attempt, k)
        d.release()


def test_fft_errors(gm):
    d = gm.fft.NewDomain("bn254", 64)
    with pytest.raises(ValueError):
        d.FFT(np.zeros((32, 4), dtype=np.uint64), gm.fft.DIF)  # len(a) != cardinality
    with pytest.raises(ValueError):
        gm.fft.BitReverse("bn254", np.zeros((24, 4), dtype=np.uint64))  # "len(a) must be a power of 2"
    d.release()


def test_fft_2_pow_22_device_resident(gm, oracle_mod):
    """BN254, 2^22 coefficients resident in HBM: DIF then the inverse DIT restores the input (fft_test.go:160-180), the
    forward result equals the oracle's, and the coset pair does the same."""
    import torch
    curve = "bn254"
    F = oracle_mod.FFT(curve)
    c = F.curve
    n = 1 << 22
    a = random_field_limbs(rng_for(82, 22), c.r, c.fr_limbs, n)
    d = gm.fft.NewDomain(curve, n)
    t = torch.from_numpy(a.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    d.fft_device(t.data_ptr(), gm.fft.DIF, stream=stream)
    got = t.cpu().numpy().view(np.uint64)
    assert (got == F.transform(a, decimation=oracle_mod.DIF)).all()
    d.fft_device(t.data_ptr(), gm.fft.DIT, inverse=True, stream=stream)
    assert (t.cpu().numpy().view(np.uint64) == a).all()
    d.fft_device(t.data_ptr(), gm.fft.DIF, gm.fft.OnCoset(), stream=stream)
    d.fft_device(t.data_ptr(), gm.fft.DIT, gm.fft.OnCoset(), inverse=True, stream=stream)
    assert (t.cpu().numpy().view(np.uint64) == a).all()
    gm.fft.BitReverse(curve, d_a=t.data_ptr(), n=n, stream=stream)
    gm.fft.BitReverse(curve, d_a=t.data_ptr(), n=n, stream=stream)
    assert (t.cpu().numpy().view(np.uint64) == a).all()
    d.release()


# ---- pass shapes of FftField::run (gmsm_fft.h) that the sizes above do not select. The low pass takes LOWB bits (10 for the
# 32-byte fields, 9 for BW6-761), the rest goes in passes of at most 8 bits (tiles of 2^B rows x 8 elements), split unequally
# when it does not divide; 512 threads per tile from 2^22 on.
def _pass_bits(curve, logn):
    """(low pass bits, [high pass bits]) as FftField::run cuts them"""
    low = min(logn, 9 if curve == "bw6_761" else 10)
    rest, out = logn - low, []
    nhi = (rest + 7) // 8
    for k in range(nhi):
        b = -(-rest // (nhi - k))
        out.append(b)
        rest -= b
    return low, out


def test_pass_shapes_named_below():
    assert [_pass_bits("bn254", lg)[1] for lg in (15, 17, 18, 19, 21)] == [[5], [7], [8], [5, 4], [6, 5]]
    assert [_pass_bits("bw6_761", lg)[1] for lg in (15, 17, 18, 19, 22)] == [[6], [8], [5, 4], [5, 5], [7, 6]]
    assert _pass_bits("bls12_381", 22)[1] == [6, 6]


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("logn", [15, 17, 18, 19])
def test_fft_matches_oracle_high_pass_shapes(gm, oracle_mod, curve, logn):
    """Single high passes of 5, 7 and 8 bits and the 5+4 split (32-byte fields), 6 and 8 bits, 5+4 and 5+5 (BW6-761); the
    8-bit pass's tile of 2^11 lazy elements is the largest dynamic-LDS request the library makes."""
    F = oracle_mod.FFT(curve)
    c = F.curve
    n = 1 << logn
    a = random_field_limbs(rng_for(85, logn, c.fr_limbs), c.r, c.fr_limbs, n)
    d = gm.fft.NewDomain(curve, n)
    for inverse in (False, True):
        for dec in (gm.fft.DIT, gm.fft.DIF):
            for coset in (False, True):
                opts = (gm.fft.OnCoset(),) if coset else ()
                got = (d.FFTInverse if inverse else d.FFT)(a, dec, *opts)
                want = F.transform(a, inverse=inverse, decimation=dec, coset=coset)
                assert (got == want).all(), (inverse, dec, coset)
    d.release()


def _device_resident(gm, oracle_mod, curve, logn, seed, oracle_coset_and_inverse):
    """The form of test_fft_2_pow_22_device_resident: forward DIF against the oracle, DIF -> inverse DIT restores the input, the
    coset pair does the same, BitReverse twice; with oracle_coset_and_inverse the coset forward and both inverse-DIT
    transforms are compared with the oracle as well."""
    import torch
    F = oracle_mod.FFT(curve)
    c = F.curve
    n = 1 << logn
    a = random_field_limbs(rng_for(seed, logn, c.fr_limbs), c.r, c.fr_limbs, n)
    d = gm.fft.NewDomain(curve, n)
    t = torch.from_numpy(a.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    host = lambda: t.cpu().numpy().view(np.uint64)
    d.fft_device(t.data_ptr(), gm.fft.DIF, stream=stream)
    fwd = host()
    assert (fwd == F.transform(a, decimation=oracle_mod.DIF)).all()
    d.fft_device(t.data_ptr(), gm.fft.DIT, inverse=True, stream=stream)
    assert (host() == a).all()
    d.fft_device(t.data_ptr(), gm.fft.DIF, gm.fft.OnCoset(), stream=stream)
    if oracle_coset_and_inverse:
        assert (host() == F.transform(a, decimation=oracle_mod.DIF, coset=True)).all()
    d.fft_device(t.data_ptr(), gm.fft.DIT, gm.fft.OnCoset(), inverse=True, stream=stream)
    assert (host() == a).all()
    if oracle_coset_and_inverse:  # the inverse DIT of a vector that is not a transform of anything: the input itself
        for coset in (False, True):
            opts = (gm.fft.OnCoset(),) if coset else ()
            assert (d.FFTInverse(a, gm.fft.DIT, *opts) == F.transform(a, inverse=True, decimation=oracle_mod.DIT, coset=coset)).all(), coset
    gm.fft.BitReverse(curve, d_a=t.data_ptr(), n=n, stream=stream)
    gm.fft.BitReverse(curve, d_a=t.data_ptr(), n=n, stream=stream)
    assert (host() == a).all()
    d.release()


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_fft_2_pow_21_unequal_split(gm, oracle_mod, curve):
    """2^21 for the 32-byte fields: 10 + 6 + 5. Forward DIF and inverse DIT, plain and on the coset, against the oracle; the
    round trips on the device buffer."""
    _device_resident(gm, oracle_mod, curve, 21, 86, True)


@pytest.mark.parametrize("curve", ["bls12_381", "bw6_761"])
def test_fft_2_pow_22_device_resident_other_fields(gm, oracle_mod, curve):
    """The 512-thread passes for the fields test_fft_2_pow_22_device_resident leaves out (BW6-761: a low tile of 256
    butterflies per stage under 512 threads, and the 7 + 6 split)."""
    _device_resident(gm, oracle_mod, curve, 22, 87, False)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_fft_class_edges_2_pow_18(gm, oracle_mod, curve):
    """The inputs of test_fft_class_edges at 2^18: an 8-bit high pass for the 32-byte fields (the most stages between two
    reductions of a high pass), the 5+4 split for BW6-761."""
    F = oracle_mod.FFT(curve)
    c = F.curve
    n = 1 << 18
    rm1 = np.array([(c.r - 1 >> (64 * k)) & (2**64 - 1) for k in range(c.fr_limbs)], dtype=np.uint64)
    fr = oracle_mod.Field(f"{c.name}_fr", c.fr_limbs)
    top = np.tile(fr.to_mont(rm1), (n, 1))  # Montgomery form of r - 1
    raw = np.tile(rm1, (n, 1))              # the limbs r - 1 themselves: the largest canonical limb pattern
    alt = raw.copy()
    alt[1::2] = 0
    spike = np.zeros_like(raw)
    spike[n // 3] = rm1
    d = gm.fft.NewDomain(curve, n)
    for a in (top, raw, alt, spike, np.zeros_like(raw)):
        for inverse in (False, True):
            for dec in (gm.fft.DIT, gm.fft.DIF):
                for coset in (False, True):
                    opts = (gm.fft.OnCoset(),) if coset else ()
                    got = (d.FFTInverse if inverse else d.FFT)(a, dec, *opts)
                    want = F.transform(a, inverse=inverse, decimation=dec, coset=coset)
                    assert (got == want).all(), (inverse, dec, coset)
    d.release()


# ---- the scalar field's entries under a G2 group id. The Python wrappers always pass the G1 id; the C ABI takes either, and
# both must reach the one table of the curve's scalar field.
@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("logn", [4, 11])
def test_scalar_field_entries_take_the_g2_id(gm, oracle_mod, curve, logn):
    """A domain made with the G2 id, then gmsm_fft (every direction, decimation and coset choice), gmsm_fft_bit_reverse,
    gmsm_poly_eval, gmsm_poly_div_x_minus_a and gmsm_fr_batch_invert with the G2 id: limb for limb what the G1 id gives, and
    the oracle's values for the transforms; gmsm_iop_to_basis on the G2-made domain equals the one on a G1-made domain.
    n = 16, and 2^11 so that a transform takes more than one pass."""
    import ctypes
    L = gm._lib.load()
    F = oracle_mod.FFT(curve)
    c = F.curve
    n, nl = 1 << logn, c.fr_limbs
    a = random_field_limbs(rng_for(88, logn, nl), c.r, nl, n)
    point = random_field_limbs(rng_for(89, logn, nl), c.r, nl, 1)[0]
    ptr = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))

    def ok(rc):
        assert rc == 0, gm._lib.last_error()

    def run(gid):
        out = {}
        h = ctypes.c_uint64(0)
        ok(L.gmsm_fft_domain_new(gid, n, ctypes.byref(h)))
        for inverse in (0, 1):
            for dec in (gm.fft.DIT, gm.fft.DIF):
                for coset in (0, 1):
                    v = a.copy()
                    ok(L.gmsm_fft(h.value, ptr(v), None, n, inverse, dec, coset, None))
                    out["fft", inverse, dec, coset] = v
        v = a.copy()
        ok(L.gmsm_fft_bit_reverse(gid, ptr(v), None, n, None))
        out["bit_reverse"] = v
        lens = (ctypes.c_size_t * 2)(n - 3, 3)
        vals = np.zeros((2, nl), dtype=np.uint64)
        ok(L.gmsm_poly_eval(gid, ptr(a), None, lens, 2, ptr(point), None, ptr(vals)))
        out["poly_eval"] = vals
        q, value = np.zeros((n - 1, nl), dtype=np.uint64), np.zeros(nl, dtype=np.uint64)
        ok(L.gmsm_poly_div_x_minus_a(gid, ptr(a), None, n, ptr(point), None, ptr(q), None, ptr(value)))
        out["poly_div"], out["poly_div_value"] = q, value
        inv = np.zeros_like(a)
        ok(L.gmsm_fr_batch_invert(gid, ptr(a), None, n, None, ptr(inv), None))
        out["batch_invert"] = inv
        v, layout = a.copy(), ctypes.c_int(0)
        ok(L.gmsm_iop_to_basis(h.value, ptr(v), None, n, gm.iop.Canonical, gm.iop.Regular, gm.iop.Lagrange, None, ctypes.byref(layout)))
        out["iop_to_basis"], out["iop_layout"] = v, np.array([layout.value])
        ok(L.gmsm_fft_domain_release(h.value))
        return out

    g1 = run(gm._lib.GROUP_IDS[(c.name, "g1")])
    g2 = run(gm._lib.GROUP_IDS[(c.name, "g2")])
    assert g1.keys() == g2.keys()
    for key in g1:
        assert (g2[key] == g1[key]).all(), key
    for inverse in (0, 1):
        for dec in (gm.fft.DIT, gm.fft.DIF):
            for coset in (0, 1):
                want = F.transform(a, inverse=bool(inverse), decimation=dec, coset=bool(coset))
                assert (g2["fft", inverse, dec, coset] == want).all(), (inverse, dec, coset)
    assert (g2["bit_reverse"] == F.bit_reverse(a)).all()
    fr = oracle_mod.Field(f"{c.name}_fr", nl)
    one = fr.to_mont(np.array([1] + [0] * (nl - 1), dtype=np.uint64))
    for i in (0, 1, n // 2, n - 1):  # (a random element is zero with probability 2^-253 at the most)
        assert (fr.mul(a[i], g2["batch_invert"][i]) == one).all(), i
