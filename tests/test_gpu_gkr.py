"""GKR on the device against the big-int model (tests/gkr_model.py), limb for limb, at the smallest shapes at which each
kernel can go wrong:
  - gmsm_multilin_fold / _evaluate / _eq: half below a wave, one wave, one workgroup, several; host pointers and device
    pointers on a non-default torch stream; the parts that must not be written
  - one sumcheck claim, round by round (claim_new, every next, final) with random challenges: every run walks half from its
    first value down to 1, so it crosses the one-workgroup / several-workgroups boundary of the reduction wherever it lies;
    n = 13 gives 16 workgroups of partial sums at the largest workgroup; BW6-761 at n = 16 over a ten-register gate (64 lanes) and
    BN254 at n = 18 (256 lanes) give 512, more than k_gkr_finish has lanes
  - the reference's eight golden proofs through gkr.Prove over a constant hash, with host and with device assignments
  - a random circuit with a sha256 transcript against the model's proof, which the model's Verify accepts
  - handle lifecycle and four threads with a claim each"""
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import gkr_model as M
import point_batch_cases as pc
from conftest import random_scalars, rng_for

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bw6_761"]
HERE = os.path.dirname(os.path.abspath(__file__))


def curve_of(gm, name):
    return gm.curves.CURVES[name]


def to_ints(c, limbs):
    rinv = pow(c.fr_R, -1, c.r)
    a = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, c.fr_limbs)
    return [int.from_bytes(row.tobytes(), "little") * rinv % c.r for row in a]


def from_ints(c, values):
    out = np.zeros((len(values), c.fr_limbs), dtype=np.uint64)
    for i, v in enumerate(values):
        out[i] = np.frombuffer((v % c.r * c.fr_R % c.r).to_bytes(c.fr_limbs * 8, "little"), dtype=np.uint64)
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda() * 1  # produced by a kernel on the current stream


def back(t, c):
    return t.cpu().numpy().view(np.uint64).reshape(-1, c.fr_limbs)


# ------------------------------------------------------------------ MultiLin
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("length", [2, 4, 128, 512, 1 << 11, 1 << 13])
def test_fold(gm, curve, length):
    import torch
    c = curve_of(gm, curve)
    rng = rng_for(0x6B01, CURVES.index(curve), length)
    a = random_scalars(rng, c, length)
    r = random_scalars(rng, c, 1)[0]
    exp = to_ints(c, a)
    M.fold(exp, to_ints(c, r)[0], c.r)
    m = gm.polynomial.MultiLin(c, a.copy())
    whole = m.values
    m.Fold(r)
    assert len(m) == length // 2 and to_ints(c, whole) == exp  # the upper half of exp is the input's
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = dev(a)
        gm.polynomial.fold_device(c, t.data_ptr(), length, r, s.cuda_stream)
    s.synchronize()
    assert to_ints(c, back(t, c)) == exp


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 7, 13])
def test_evaluate(gm, curve, n):
    import torch
    c = curve_of(gm, curve)
    rng = rng_for(0x6B02, CURVES.index(curve), n)
    a = random_scalars(rng, c, 1 << n)
    ints = to_ints(c, a)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = dev(a)
    for ncoords in sorted({0, 1, n - 1, n}):
        coords = random_scalars(rng, c, ncoords)
        exp = M.evaluate(ints, to_ints(c, coords), c.r)
        m = gm.polynomial.MultiLin(c, a.copy())
        assert to_ints(c, m.Evaluate(coords)) == [exp]
        assert (m.values == a).all()
        with torch.cuda.stream(s):
            assert to_ints(c, gm.polynomial.evaluate_device(c, t.data_ptr(), 1 << n, coords, s.cuda_stream)) == [exp]
    s.synchronize()
    assert (back(t, c) == a).all()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [0, 1, 2, 6, 7, 9, 13])
def test_eq(gm, curve, n):
    import torch
    c = curve_of(gm, curve)
    rng = rng_for(0x6B03, CURVES.index(curve), n)
    q = random_scalars(rng, c, n)
    scale = random_scalars(rng, c, 1)[0]
    exp = M.eq_loop([to_ints(c, scale)[0]] + [0] * ((1 << n) - 1), to_ints(c, q), c.r)
    m = gm.polynomial.MultiLin(c, np.concatenate([scale.reshape(1, -1), random_scalars(rng, c, (1 << n) - 1)]))  # only m[0] is read
    m.Eq(q)
    assert to_ints(c, m.values) == exp
    # accumulate onto a random table, on the device
    base = random_scalars(rng, c, 1 << n)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = dev(base)
        gm.polynomial.eq_device(c, q, scale, t.data_ptr(), accumulate=True, stream=s.cuda_stream)
        t2 = dev(base)
        gm.polynomial.eq_device(c, q, scale, t2.data_ptr(), accumulate=False, stream=s.cuda_stream)
    s.synchronize()
    assert to_ints(c, back(t, c)) == [(x + y) % c.r for x, y in zip(to_ints(c, base), exp)]
    assert to_ints(c, back(t2, c)) == exp
    if n:
        # a boolean point: exactly one entry is scale, the others 0
        h = int(rng.integers(0, 1 << n))
        qb = from_ints(c, [(h >> (n - 1 - i)) & 1 for i in range(n)])
        m = gm.polynomial.MultiLin(c, np.concatenate([scale.reshape(1, -1), np.zeros(((1 << n) - 1, c.fr_limbs), dtype=np.uint64)]))
        m.Eq(qb)
        got = to_ints(c, m.values)
        assert got[h] == to_ints(c, scale)[0] and sum(1 for v in got if v) == 1
        # a zero coordinate
        qz = q.copy()
        qz[n // 2] = 0
        m = gm.polynomial.MultiLin(c, np.concatenate([scale.reshape(1, -1), np.zeros(((1 << n) - 1, c.fr_limbs), dtype=np.uint64)]))
        m.Eq(qz)
        assert to_ints(c, m.values) == M.eq_closed(to_ints(c, qz), to_ints(c, scale)[0], c.r)


# ------------------------------------------------------------------ one claim, round by round
def mimc(x, y):
    s = x + y
    s3 = s * s * s
    return s3 * s3 * s


def add8(*x):
    r = x[0]
    for v in x[1:]:
        r = r + v
    return r


def wide8(*x):
    """8 inputs, degree 8, 16 live registers: the 8 sums stay live across the product of all inputs"""
    t = [x[j] + x[(j + 1) % 8] for j in range(8)]
    p = x[0]
    for v in x[1:]:
        p = p * v
    r = p + t[0] * t[1]
    r = r + t[2] * t[3]
    r = r + t[4] * t[5]
    return r + t[6] * t[7]


# name -> (callable, inputs, declared degree, same pointer for every input)
GATES = {
    "identity": (lambda x: x, 1, 1, False),
    "mul_same": (lambda x, y: x * y, 2, 2, True),
    "mimc": (mimc, 2, 7, False),
    "add8": (add8, 8, 1, False),
    "wide8": (wide8, 8, 8, False),
    "deg3_as_5": (lambda x, y: x * y * y + x, 2, 5, False),
    "pairs8": (pc.pairs8, 8, 2, False),
}


def test_wide_gate_uses_sixteen_registers(gm):
    code = gm.gkr.Gate(wide8, 8).code("bn254", 8)
    assert max((int(w) >> 8) & 0xFF for w in code.words) == 15


def run_claim(gm, c, name, n, k, rng, device, stream=0):
    """claim_new, every next, final against the model; returns the device's bytes of all rounds"""
    f, m, degree, same = GATES[name]
    tables = [random_scalars(rng, c, 1 << n) for _ in range(1 if same else m)]
    if same:
        tables = tables * m
    points = [random_scalars(rng, c, n) for _ in range(k)]
    comb = random_scalars(rng, c, 1)[0]
    model = M.Claim(c.r, M.Gate(f, degree), [to_ints(c, t) for t in tables], [to_ints(c, p) for p in points])
    keep = [t.copy() for t in tables]
    if device:
        dts = [dev(t) for t in tables[:1 if same else m]]
        if same:
            dts = dts * m
        handles = [t.data_ptr() for t in dts]
    else:
        handles = tables
    claim = gm.gkr.Claim(c, gm.gkr.Gate(f, degree), handles, 1 << n, points, device=device, stream=stream)
    got = []
    try:
        gj = claim.Combine(comb)
        got.append(gj.copy())
        assert to_ints(c, gj) == model.combine(to_ints(c, comb)[0]), "first round"
        for j in range(n - 1):
            r = random_scalars(rng, c, 1)[0]
            gj = claim.Next(r)
            got.append(gj.copy())
            assert to_ints(c, gj) == model.next(to_ints(c, r)[0]), "round %d" % (j + 1)
        r = random_scalars(rng, c, 1)[0]
        ev = claim.final(r)
        got.append(ev.copy())
        assert to_ints(c, ev) == model.final_fold(to_ints(c, r)[0])
    finally:
        claim.release()
    if device:
        import torch
        torch.cuda.synchronize()
        for t, orig in zip(dts, keep):
            assert (back(t, c) == orig).all(), "the caller's device tables were modified"
    for t, orig in zip(tables, keep):
        assert (t == orig).all(), "the caller's tables were modified"
    return b"".join(g.tobytes() for g in got)


def claim_cases():
    for curve in CURVES:
        for name in GATES:
            if name == "wide8" and curve == "bls12_381":
                continue  # the smallest and the largest element size
            if name == "pairs8":
                continue  # the gate of test_claim_with_more_workgroups_than_lanes: wide8 has its register pressure at these sizes
            for n in (1, 2, 6, 7, 8, 9, 10, 13):
                yield curve, name, n


@pytest.mark.parametrize("curve,name,n", list(claim_cases()))
def test_claim_round_by_round(gm, curve, name, n):
    c = curve_of(gm, curve)
    for k in (1, 2, 3):
        rng = rng_for(0x6B04, CURVES.index(curve), list(GATES).index(name), n, k)
        run_claim(gm, c, name, n, k, rng, device=(k + n) % 2 == 0)


def test_pairs_gate_leaves_sixty_four_lanes(gm):
    """10 registers and the row of wave sums of 48-byte elements: 11 x 48 x 128 bytes exceed the round kernel's LDS budget"""
    code = gm.gkr.Gate(pc.pairs8, 2).code("bw6_761", 8)
    assert max((int(w) >> 8) & 0xFF for w in code.words) >= 9


MANY_WORKGROUPS = pc.MANY_WORKGROUPS  # (curve, gate, n, k, lanes of the round kernel): 512 workgroups in the first round


@pytest.mark.parametrize("curve,name,n,k,lanes", MANY_WORKGROUPS, ids=[f"{c}-{g}-{n}-{k}" for c, g, n, k, _ in MANY_WORKGROUPS])
def test_claim_with_more_workgroups_than_lanes(gm, curve, name, n, k, lanes):
    """The first round's 512 rows of partial sums are twice the lanes of k_gkr_finish, whose strided loop takes a second step
    (and in the next round, at 256 rows, exactly one); the claim then halves its way down through 128 .. 2 workgroups to the
    single-workgroup rounds that need no second launch (tests/test_point_batch_cases.py derives the counts from the host code)."""
    c = curve_of(gm, curve)
    assert (1 << (n - 1)) // lanes == 512
    rng = rng_for(0x6B09, CURVES.index(curve), list(GATES).index(name), n, k)
    run_claim(gm, c, name, n, k, rng, device=(k + n) % 2 == 0)


@pytest.mark.parametrize("curve", CURVES)
def test_claim_is_deterministic(gm, curve):
    c = curve_of(gm, curve)
    runs = [run_claim(gm, c, "mimc", 10, 2, rng_for(0x6B05, CURVES.index(curve)), device=True) for _ in range(2)]
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ whole proofs
MODEL_TO_DEVICE = {"identity": "identity", "add": "add", "sub": "sub", "neg": "neg", "mul": "mul"}


def device_gate(gm, name):
    if name in MODEL_TO_DEVICE:
        return gm.gkr.Gates[name]
    return {"mimc": gm.gkr.Gate(mimc, 7), "select-input-3": gm.gkr.Gate(lambda *x: x[2], 1)}[name]


def build_circuit(gm, circuit):
    wires = gm.gkr.Circuit(gm.gkr.Wire() for _ in circuit)
    for w, (g, ins) in zip(wires, circuit):
        if ins:
            w.Gate = g if isinstance(g, gm.gkr.Gate) else device_gate(gm, g)
            w.Inputs = [wires[j] for j in ins]
    return wires


def prove_on_device(gm, c, circuit, inputs, hash_factory, device):
    """inputs: circuit index -> ints. Returns (proof as ints, completed assignment as ints per circuit index)."""
    wires = build_circuit(gm, circuit)
    n = len(next(iter(inputs.values())))
    arrays = {j: from_ints(c, v) for j, v in inputs.items()}
    if device:
        tensors = {j: dev(a) for j, a in arrays.items()}
        a = gm.gkr.WireAssignment(c, {wires[j]: t.data_ptr() for j, t in tensors.items()}, nb_instances=n, device=True)
    else:
        a = gm.gkr.WireAssignment(c, {wires[j]: v for j, v in arrays.items()})
    a.Complete(wires)
    proof = gm.gkr.Prove(wires, a, gm.fiatshamir.WithHash(hash_factory))
    full = [to_ints(c, a.to_host(w)) if not w.IsInput() else inputs[j] for j, w in enumerate(wires)]
    out = [{"partialSumPolys": [to_ints(c, p) for p in pw.PartialSumPolys], "finalEvalProof": [to_ints(c, e)[0] for e in pw.FinalEvalProof]}
           for pw in proof]
    return out, full


class ConstHash:
    def __init__(self, c, val):
        self.out = (val % c.r).to_bytes(c.fr_limbs * 8, "big")

    def update(self, b):
        pass

    def digest(self):
        return self.out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("device", [False, True])
def test_reference_vectors(gm, curve, device):
    c = curve_of(gm, curve)
    F = M.Field(c.r, c.fr_limbs * 8)
    with open(os.path.join(HERE, "golden", "gkr_vectors.json")) as f:
        vectors = json.load(f)
    assert len(vectors) == 8
    for name, v in vectors.items():
        circuit = [(g, ins) for g, ins in v["circuit"]]
        s = M.Sorted(circuit)
        ins, outs = iter(v["input"]), iter(v["output"])
        inputs, expected_out = {}, {}
        for w in s.order:
            if s.is_input(w):
                inputs[w] = [x % F.p for x in next(ins)]
            elif s.is_output(w):
                expected_out[w] = [x % F.p for x in next(outs)]
        proof, full = prove_on_device(gm, c, circuit, inputs, lambda: ConstHash(c, v["hash"]["val"]), device)
        expected = [{"partialSumPolys": [[x % F.p for x in poly] for poly in pw["partialSumPolys"]],
                     "finalEvalProof": [x % F.p for x in (pw["finalEvalProof"] or [])]} for pw in v["proof"]]
        assert proof == expected, name
        if full is not None:
            for w, out in expected_out.items():
                assert full[w] == out, name


@pytest.mark.parametrize("curve", CURVES)
def test_end_to_end_with_sha256(gm, curve):
    """a three-level MiMC chain over inputs 0 and 1; input 0 feeds every level, so it has several claims and a comb challenge;
    the last wire multiplies the chain's end by itself (a repeated input)"""
    c = curve_of(gm, curve)
    F = M.Field(c.r, c.fr_limbs * 8)
    rng = rng_for(0x6B06, CURVES.index(curve))
    n = 1 << 9
    circuit = [(None, []), (None, []), ("mimc", [1, 0]), ("mimc", [2, 0]), ("mimc", [3, 0]), ("mul", [4, 4])]
    inputs = {j: to_ints(c, random_scalars(rng, c, n)) for j in (0, 1)}
    full = M.complete(circuit, [inputs[0], inputs[1], None, None, None, None], F.p)
    expected = M.prove(F, circuit, full, hashlib.sha256)
    assert any(name.endswith("comb") for name in M.challenge_names(M.Sorted(circuit), 9))
    for device in (False, True):
        proof, got_full = prove_on_device(gm, c, circuit, inputs, hashlib.sha256, device)
        assert proof == expected
        if got_full is not None:
            assert got_full == full
    assert M.verify(F, circuit, full, proof, hashlib.sha256) is None


# ------------------------------------------------------------------ lifecycle and threads
def test_lifecycle_refusals_leave_the_gpu_usable(gm):
    c = curve_of(gm, "bn254")
    rng = rng_for(0x6B07)
    lib = gm._lib.load()
    tables = [random_scalars(rng, c, 4) for _ in range(2)]
    points = [random_scalars(rng, c, 2)]
    r = random_scalars(rng, c, 1)[0]
    claim = gm.gkr.Claim(c, gm.gkr.Gates["mul"], tables, 4, points)
    claim.Combine(r)
    with pytest.raises(ValueError, match="not 2"):
        claim.final(r)
    claim.Next(r)
    with pytest.raises(ValueError, match="no variable is left"):
        claim.Next(r)
    claim.final(r)
    with pytest.raises(ValueError, match="the claim is finished"):
        claim.final(r)
    with pytest.raises(ValueError, match="the claim is finished"):
        claim.Next(r)
    handle = claim.handle
    claim.release()
    assert lib.gmsm_gkr_claim_release(handle) != 0 and gm._lib.last_error() == "unknown gkr claim handle"
    claim.handle = handle
    with pytest.raises(ValueError, match="unknown gkr claim handle"):
        claim.Next(r)
    claim.handle = None
    run_claim(gm, c, "mimc", 6, 1, rng, device=False)  # the GPU is still usable


def test_four_threads_with_a_claim_each(gm):
    import torch
    c = curve_of(gm, "bn254")
    errors = []

    def work(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for i in range(3):
                    run_claim(gm, c, "mimc", 8, 2, rng_for(0x6B08, t, i), device=True, stream=s.cuda_stream)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
