"""Bucket contents for the tests of the bucket reduction (tests/test_reduce_cases_model.py on the host model of
tests/combine_model.py, tests/test_gpu_reduce_shapes.py on the device): for a launch shape (NB buckets, L = 2^log2L buckets
per serial segment, two or three levels) named cases of integers b[w][j] mod r - bucket j of bucket set w holds [b]G, 0 =
empty - and a flag per bucket "stored but infinite" (a record the accumulation wrote with zz = 0: P and -P met in it).

Where a case is named for a collision, the values are solved for from the shape: everything is linear mod r.
    dense             random values, every bucket occupied
    sparse            about one bucket in eight occupied
    all_equal         b = 1 everywhere: S_t = L for every full segment, so every step of a suffix scan (and of the pair sums
                      of k_combine_we) adds equal operands
    alternating       +k, -k, +k', -k' ... in every serial segment: the running sum returns to infinity after every pair,
                      every S_t is infinite while W_t is not
    zero_S            the buckets of every first-level combine block sum to 0 while their weighted sum does not: the parked
                      S_blk is infinite, and so is every sum of S above it
    zero_total        sum (j + 1) b_j = 0: the window total is infinity
    single@j          one occupied bucket, at the seams of a serial segment, a combine block and the last bucket:
                      j in 0, L-1, L, 64L-1, 64L, NB-1 (those that exist)
    finish+ finish-   buckets 0 and L hold x = (+-L - 1) y and y: the last step of the first combine, W + L U, is P + P / P - P
    finish2+ finish2- the same one level up (NB > 64 L + 1). Three levels: buckets 0 and 64L hold x = (+-64L - 1) y and y, the
                      last step of the second combine is P + P / P - P. Two levels: k_reduce2_q adds the scaled suffix quad by
                      quad, W_j + Suf_j, so the collision is solved for inside block 1 - buckets 64L and 64L + 1 hold y and z
                      with y + 2 z = +-64L (y + z) - and for the sign + bucket 0 holds W_1 + Suf_1, which makes the step of the
                      tree over the quads that adds quads 0 and 1 a P + P too
    stored_infinity   random values with stored-but-infinite buckets at the first slot, the last slot and (L >= 4) a middle
                      slot of the first, the second and the last segment, and one between two finite buckets"""
import random

from combine_model import COMBINE_N, RED2_TPB

C_VALUES = (2, 7, 11, 14)   # NB = 2^(c-1) = 2, 64, 1024, 8192
LOG2LS = (1, 2, 4, 8)
SPARSE_ONE_IN = 8


def nbuckets(fr_bits, c):
    """buckets of one bucket set at width c (Group::make_plan; lastC of multiexp.go:690): 2^(max(c, lastC) - 1). Only the top
    window can reach past 2^(c-1): the sets are larger than that where c divides the bit length of r."""
    nwin = (fr_bits + c - 1) // c
    return 1 << (max(c, c + 1 - (nwin * c - fr_bits)) - 1)


def admissible(NB, log2L, levels):
    """what the planner can run without raising log2L: two levels need NB <= 64 * 64 L, three need a second block (NB > 64 L)"""
    L = 1 << log2L
    return NB <= RED2_TPB * COMBINE_N * L if levels == 2 else NB > COMBINE_N * L


def shapes(NB):
    return [(l2, lv) for lv in (2, 3) for l2 in LOG2LS if admissible(NB, l2, lv)]


class Case:
    def __init__(self, name, b, inf):
        self.name, self.b, self.inf = name, b, inf

    def key(self):
        """contents as a hashable value: cases of different shapes with the same contents share their expected results"""
        return (tuple(tuple(w) for w in self.b), tuple(tuple(w) for w in self.inf))


def weighted(r, b):
    return sum((j + 1) * v for j, v in enumerate(b)) % r


def cases(r, NB, log2L, levels, nw):
    L, N = 1 << log2L, COMBINE_N
    span = N * L
    inv = lambda v: pow(v % r, -1, r)
    out = {}

    def make(name, fill, tag=""):
        bs, infs = [], []
        for w in range(nw):
            rng = random.Random(f"{name}/{r}/{NB}/{tag}/{w}")
            b, inf = [0] * NB, [False] * NB
            fill(rng, b, inf)
            assert all(0 <= v < r for v in b) and not any(i and v for i, v in zip(inf, b))
            bs.append(b)
            infs.append(inf)
        out[name] = Case(name, bs, infs)

    rnd = lambda rng: rng.randrange(1, r)

    def dense(rng, b, inf):
        b[:] = [rnd(rng) for _ in range(NB)]
    make("dense", dense)

    def sparse(rng, b, inf):
        hit = [j for j in range(NB) if rng.randrange(SPARSE_ONE_IN) == 0] or [rng.randrange(NB)]
        for j in hit:
            b[j] = rnd(rng)
    make("sparse", sparse)

    def all_equal(rng, b, inf):
        b[:] = [1] * NB
    make("all_equal", all_equal)

    def alternating(rng, b, inf):
        for j in range(0, NB, 2):  # L and NB are even: every pair lies inside one segment
            k = rnd(rng)
            b[j], b[j + 1] = k, r - k
    make("alternating", alternating)

    def zero_S(rng, b, inf):
        dense(rng, b, inf)
        for lo in range(0, NB, span):
            hi = min(lo + span, NB)
            b[hi - 1] = -sum(b[lo:hi - 1]) % r
    make("zero_S", zero_S, tag=f"L{L}")

    def zero_total(rng, b, inf):
        dense(rng, b, inf)
        b[0] = -weighted(r, [0] + b[1:]) % r
    make("zero_total", zero_total)

    for j in sorted({0, L - 1, L, span - 1, span, NB - 1}):
        if j < NB:
            def single(rng, b, inf, j=j):
                b[j] = rnd(rng)
            make(f"single@{j}", single)

    if L < NB:
        for sign, tag in ((1, "+"), (-1, "-")):
            def finish(rng, b, inf, sign=sign):
                y = rnd(rng)
                b[L], b[0] = y, (sign * L - 1) * y % r
            make("finish" + tag, finish, tag=f"L{L}")
    if span + 1 < NB:
        for sign, tag in ((1, "+"), (-1, "-")):
            def finish2(rng, b, inf, sign=sign):
                if levels == 3:
                    y = rnd(rng)
                    b[span], b[0] = y, (sign * span - 1) * y % r
                else:  # W_1 = y + 2 z, Suf_1 = span (y + z): y (1 - sign span) = z (sign span - 2)
                    z = rnd(rng)
                    y = z * (sign * span - 2) * inv(1 - sign * span) % r
                    b[span], b[span + 1] = y, z
                    w1, suf1 = (y + 2 * z) % r, span * (y + z) % r
                    assert w1 == sign * suf1 % r and y
                    b[0] = (w1 + suf1) % r if sign > 0 else rnd(rng)  # (sign -: quad 1 is left infinite, nothing to meet)
            make("finish2" + tag, finish2, tag=f"L{L}/{levels}")

    def stored_infinity(rng, b, inf):
        dense(rng, b, inf)
        T = (NB + L - 1) // L
        for t in sorted({0, min(1, T - 1), T - 1}):
            lo, hi = t * L, min((t + 1) * L, NB)
            for j in {lo, hi - 1} | ({lo + L // 2} if L >= 4 and lo + L // 2 < hi - 1 else set()):
                b[j], inf[j] = 0, True
        if T > 4:  # L <= 4 leaves no slot with finite buckets on both sides inside those segments: the first slot of segment 3
            b[3 * L], inf[3 * L] = 0, True
        if all(inf):  # NB = 2: keep a finite bucket
            b[1], inf[1] = rnd(rng), False
    make("stored_infinity", stored_infinity, tag=f"L{L}")
    return out
