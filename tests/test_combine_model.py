"""Lockstep model (tests/combine_model.py) of the quad step machines of the bucket reduction (gmsm_quad.h: k_combine_q and its work-efficient twin
k_combine_we, the level-1 combine of the reduction, and k_reduce2_q, level 2) over the additive group Z (add = +, dbl = *2, infinity = None): every step
is "all quads read their operands - barrier - compute and store - barrier", records may be one quad's destination and
another quad's source in the same step, and the result must be
    W_blk = sum W_t + L * sum_{t>=1} Suf_t,   S_blk = 2^prescale * sum S_t        (level 1)
    total = sum_j W_j + 2^log2span * sum_{j>=1} Suf_j                              (level 2)
- the identity of multiexp_jacobian.go:44-52 cut into segments. Pure Python; it pins the index arithmetic, the parking of
S_blk and the schedule of the prescaling doublings of the device code, which the GPU suite then runs on curve points."""
import random

from combine_model import combine_q, combine_we, reduce2_q, val


def test_combine_q_identity():
    rng = random.Random(20260925)
    for N in (16, 32, 64, 128):
        lg = N.bit_length() - 1
        for log2L in (1, 2, 3, 4, 8):
            for prescale in (0, log2L + lg):  # log2span = log2L + log2 N, as the host passes it
                for _ in range(10):
                    S = [rng.randrange(1, 1 << 40) if rng.random() < 0.8 else None for _ in range(N)]
                    W = [rng.randrange(1, 1 << 40) if rng.random() < 0.9 else None for _ in range(N)]
                    s_blk, w_blk = combine_q(N, log2L, prescale, S, W)
                    suf = [sum(val(x) for x in S[t:]) for t in range(N)]
                    assert val(w_blk) == sum(val(x) for x in W) + (1 << log2L) * sum(suf[1:])
                    assert val(s_blk) == sum(val(x) for x in S) << prescale


def test_combine_we_identity():
    rng = random.Random(31)
    N = 64
    for log2L in (1, 2, 3, 4, 8):
        for prescale in (0, log2L + 6):
            for _ in range(20):
                S = [rng.randrange(1, 1 << 40) if rng.random() < 0.8 else None for _ in range(N)]
                W = [rng.randrange(1, 1 << 40) if rng.random() < 0.9 else None for _ in range(N)]
                s_blk, w_blk = combine_we(log2L, prescale, S, W)
                suf = [sum(val(x) for x in S[t:]) for t in range(N)]
                assert val(w_blk) == sum(val(x) for x in W) + (1 << log2L) * sum(suf[1:])
                assert val(s_blk) == sum(val(x) for x in S) << prescale


def test_reduce2_q_identity():
    rng = random.Random(7)
    for active in (2, 4, 16, 64):
        for nblocks1 in {1, 2, active // 2 + 1, active} & set(range(1, active + 1)):
            for log2span in (0, 3, 11):
                S = [rng.randrange(1, 1 << 40) if rng.random() < 0.8 else None for _ in range(active)]
                W = [rng.randrange(1, 1 << 40) for _ in range(active)]
                got = reduce2_q(active, nblocks1, log2span, S, W)
                suf = [sum(val(x) for x in S[j:nblocks1]) for j in range(nblocks1)]
                assert val(got) == sum(val(x) for x in W[:nblocks1]) + (1 << log2span) * sum(suf[1:])
