"""The schedule of gmsm_group_fft.h (ToLagrangeG1 on the device) restated over integers mod r, without a GPU.

G1 is cyclic of prime order r and the transform is linear, so a point [k]G can stand for its scalar k: a schedule that is
right on scalars is right on points. For every scalar field and n = 2^0 .. 2^12 this checks the kernels' plan - the
twiddle table (w^-j, w^-i / n, 1/n), the thread -> (block, i) mapping of both stage classes, the twiddle index of every
butterfly, the skip of twiddle 1, the 1/n folded into stage 0 and the bit-reversed store of the last stage - against a
restatement of the reference (difFFTG1 + bitReverse + the 1/n scaling, ecc/bn254/kzg/utils.go:25-180) and against the
closed form [L_i(tau)]G of an SRS [tau^j]G. It also checks that the wave-uniform stages give the 64 lanes of a wave one
twiddle, and that every stage reads and writes each record exactly once."""
import importlib
import random

import pytest

gm = importlib.import_module("gnark-crypto_amd")
CURVES = ["bn254", "bls12_381", "bw6_761"]
LOGS = list(range(0, 13))
WAVE = 64
UNIFORM_FROM = 6  # stages s with 2^s >= 64 blocks map a wave to 64 blocks at one i


def generator(c, log2n):
    """fr.Generator(2^log2n) (fr/generator.go)"""
    return pow(c.fr_root_of_unity, 1 << (c.fr_max_order - log2n), c.r)


def reference(c, k):
    """ToLagrangeG1 of [k_j]G as the reference computes it, on the scalars"""
    r, n = c.r, len(k)
    log2n = n.bit_length() - 1
    winv = pow(generator(c, log2n), -1, r)
    tw = [pow(winv, j, r) for j in range(1 + (n >> 1))]  # computeTwiddlesInv
    a = list(k)

    def dif(lo, size, stage):
        if size == 1:
            return
        m = size >> 1
        stride = 1 << stage
        for i in range(m):  # butterflyG1, then ScalarMultiplication by twiddles[i * stride] for i >= 1
            x, y = a[lo + i], a[lo + i + m]
            a[lo + i], a[lo + i + m] = (x + y) % r, (x - y) % r
            if i:
                a[lo + i + m] = a[lo + i + m] * tw[i * stride] % r
        if m == 1:
            return
        dif(lo, m, stage + 1)
        dif(lo + m, m, stage + 1)

    dif(0, n, 0)
    rev = [a[bitrev(i, log2n)] for i in range(n)]  # bitReverse
    ninv = pow(n, -1, r)
    return [v * ninv % r for v in rev]


def bitrev(i, log2n):
    return int(format(i, f"0{log2n}b")[::-1], 2) if log2n else 0


def twiddle_table(c, log2n):
    """k_group_fft_twiddles: e < half: w^-e; e < 2 half: w^-(e - half) / n; e = 2 half: 1/n"""
    r, n = c.r, 1 << log2n
    half = n >> 1
    winv = pow(generator(c, log2n), -1, r) if log2n else 1
    ninv = pow(n, -1, r)
    return [pow(winv, e, r) for e in range(half)] + [ninv * pow(winv, e, r) % r for e in range(half)] + [ninv]


def stage_plan(log2n, s):
    """k_group_fft_stage, stage s: per thread t the butterfly (pa, pb), which output it multiplies, the twiddle index
    (None: twiddle 1, no product) and the store positions"""
    n = 1 << log2n
    half = n >> 1
    first = s == 0
    jobs = n if first else half
    log2m = log2n - 1 - s
    last = s + 1 == log2n
    out = []
    for t in range(jobs):
        sum_job = t >= half
        bt = t - half if sum_job else t
        if s >= UNIFORM_FROM:
            k, i = bt & ((1 << s) - 1), bt >> s
        else:
            k, i = bt >> log2m, bt & ((1 << log2m) - 1)
        pa = (k << (log2m + 1)) | i
        pb = pa + (1 << log2m)
        twi = 2 * half if sum_job else (half + i if first else i << s)
        if not first and twi == 0:
            twi = None
        px = pa if sum_job else pb
        pos = (lambda p: bitrev(p, log2n)) if last else (lambda p: p)
        out.append(dict(pa=pa, pb=pb, sum_job=sum_job, twi=twi, store_x=pos(px), store_a=None if first else pos(pa)))
    return out


def buffers(log2n):
    """Group::to_lagrange: (src, dst) of every stage - stage 0 out of place, the later stages in place, the last one into
    the normalisation's input (ws.buckets)"""
    loaded = "recs" if log2n == 1 else "buckets"
    return loaded, [(loaded if s == 0 else "recs", "buckets" if s + 1 == log2n else "recs") for s in range(log2n)]


def kernel_schedule(c, k, order=1):
    """The device's flow: load, stages 0 .. log2n - 1, normalisation. Threads run one after the other (ascending t, or
    descending for order = -1) writing straight into their buffers, so a thread that overwrote what another one of the
    same stage still had to read would show up as a wrong result."""
    r, n = c.r, len(k)
    log2n = n.bit_length() - 1
    loaded, plan = buffers(log2n)
    mem = {"recs": [None] * n, "buckets": [None] * n}
    mem["buckets" if log2n == 0 else loaded] = list(k)
    if log2n == 0:
        return mem["buckets"]
    tw = twiddle_table(c, log2n)
    for s, (src, dst) in enumerate(plan):
        written = []
        for p in stage_plan(log2n, s)[::order]:
            a, b = mem[src][p["pa"]], mem[src][p["pb"]]
            x = (a + b) % r if p["sum_job"] else (a - b) % r
            if p["twi"] is not None:
                x = x * tw[p["twi"]] % r
            if p["store_a"] is not None:
                mem[dst][p["store_a"]] = (a + b) % r
                written.append(p["store_a"])
            mem[dst][p["store_x"]] = x
            written.append(p["store_x"])
        assert sorted(written) == list(range(n)), "every record written exactly once per stage"
    return mem["buckets"]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log2n", LOGS)
def test_schedule_matches_reference_and_closed_form(curve, log2n):
    c = gm.CURVES[curve]
    r, n = c.r, 1 << log2n
    rnd = random.Random(log2n * 7 + CURVES.index(curve))
    k = [rnd.randrange(r) for _ in range(n)]
    if n > 2:
        k[1] = 0  # a point at infinity
    assert kernel_schedule(c, k) == reference(c, k) == kernel_schedule(c, k, order=-1)
    tau = rnd.randrange(1, r)
    srs = [pow(tau, j, r) for j in range(n)]
    w = generator(c, log2n)
    ninv = pow(n, -1, r)
    # L_i(tau) = (1/n) sum_j x^j, x = tau w^-i: (1/n)(tau^n - 1)/(x - 1), or 1 where x = 1
    winv, tn = pow(w, -1, r), pow(tau, n, r)
    closed = []
    for i in range(n):
        x = tau * pow(winv, i, r) % r
        closed.append(1 if x == 1 else ninv * (tn - 1) * pow(x - 1, -1, r) % r)
    assert kernel_schedule(c, srs) == closed


@pytest.mark.parametrize("curve", CURVES)
def test_all_equal_input_gives_point_then_infinities(curve):
    c = gm.CURVES[curve]
    for log2n in (1, 3, 7):
        out = kernel_schedule(c, [12345] * (1 << log2n))
        assert out == [12345] + [0] * ((1 << log2n) - 1)


@pytest.mark.parametrize("log2n", LOGS)
def test_stage_classes_and_twiddle_indices(log2n):
    n = 1 << log2n
    half = n >> 1
    for s in range(log2n):
        plan = stage_plan(log2n, s)
        assert len(plan) == (n if s == 0 else half)
        reads = sorted([p["pa"] for p in plan[:half]] + [p["pb"] for p in plan[:half]])
        assert reads == list(range(n))
        for p in plan:
            assert p["pb"] - p["pa"] == n >> (s + 1)  # the DIF pair of stage s
            i = p["pa"] & ((n >> (s + 1)) - 1)
            if s == 0:
                assert p["twi"] == (2 * half if p["sum_job"] else half + i)  # 1/n folded in
            else:
                assert p["twi"] == (None if i == 0 else i << s) and (p["twi"] is None or p["twi"] < half)
        if s >= UNIFORM_FROM:  # one twiddle per wave; the waves of i = 0 skip as a whole
            for w0 in range(0, len(plan), WAVE):
                assert len({p["twi"] for p in plan[w0:w0 + WAVE]}) == 1
        elif s == 0 and half >= WAVE:  # the 1/n products of stage 0 are whole waves too
            for w0 in range(half, n, WAVE):
                assert {p["twi"] for p in plan[w0:w0 + WAVE]} == {2 * half}


def test_stage0_is_out_of_place():
    """two threads read each pair of stage 0 (b' and the 1/n product of a'): its source is not its destination"""
    for log2n in range(1, 13):
        _, plan = buffers(log2n)
        assert plan[0][0] != plan[0][1]
        assert all(src == dst for src, dst in plan[1:-1])
        assert plan[-1][1] == "buckets"


def test_twiddle_table_is_reference_twiddles():
    """computeTwiddlesInv's entries w^-j, j <= n/2 (the reference's last entry, j = n/2, is never read)"""
    c = gm.CURVES["bn254"]
    for log2n in range(1, 9):
        n = 1 << log2n
        tw = twiddle_table(c, log2n)
        winv = pow(generator(c, log2n), -1, c.r)
        assert tw[:n // 2] == [pow(winv, j, c.r) for j in range(n // 2)]
        assert pow(generator(c, log2n), n, c.r) == 1 and (log2n == 0 or pow(generator(c, log2n), n // 2, c.r) != 1)
