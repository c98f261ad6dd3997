"""Host model of the bucket reduction (gmsm_kernels.h: k_reduce_serial / k_reduce_serial_q; gmsm_quad.h: k_combine_q, its
work-efficient twin k_combine_we and k_reduce2_q): the step machines of the device code, statement for statement, over an
additive group in which an element is an integer and infinity is None.

The group is Z (Group(), what tests/test_combine_model.py pins the index arithmetic with: add = +, dbl = * 2) or Z_r
(Group(r): a sum that is 0 mod r is infinity - the scalars of curve points [b]G, so P + P, P - P and infinite operands turn
up exactly where they do on the device). A Group keeps an event log: one entry (kernel, phase, step, kind) for every
addition a quad or a lane performs and for every doubling,
    kind   'P+Q'  two finite operands, different x        'P+P'  x == y (the doubling branch of the addition)
           'P-P'  x == -y (the result is infinity)        'inf+Q' / 'P+inf' / 'inf+inf'  an infinite operand
           'dbl'  a doubling of a finite record           'dbl_inf'  a doubler that found infinity (the device skips it)
    kernel 'serial', 'combine1', 'combine2', 'reduce2'
    phase  serial: 'run', 'tot' - k_combine_q: 'scan', 'tree', 'lu' (the doublings of U), 'finish' (W + L U), 'park' -
           k_combine_we: 'pairs', 'tail', 'lu', 'finish', 'park' - k_reduce2_q: 'scan', 'span', 'finish', 'tree'
Every step is "all quads read their operands - barrier - compute and store - barrier": records may be one quad's
destination and another quad's source in the same step. The results must be
    W_blk = sum W_t + L * sum_{t>=1} Suf_t,   S_blk = 2^prescale * sum S_t        (level 1)
    total = sum_j W_j + 2^log2span * sum_{j>=1} Suf_j                              (level 2)
- the identity of multiexp_jacobian.go:44-52 cut into segments."""

COMBINE_N = 64   # Group::COMBINE_N
RED2_TPB = 64    # Group::RED2_TPB


class Group:
    def __init__(self, r=None, log=False):
        self.r = r
        self.events = [] if log else None
        self.where = ("", "", 0)

    def at(self, kernel, phase, step=0):
        self.where = (kernel, phase, step)

    def _note(self, kind, phase=None):
        if self.events is not None:
            k, p, s = self.where
            self.events.append((k, phase or p, s, kind))

    def norm(self, x):
        if self.r is None or x is None:
            return x
        x %= self.r
        return x if x else None

    def add(self, x, y, phase=None):  # group law with infinity
        if self.events is not None:
            if x is None or y is None:
                kind = "inf+inf" if x is None and y is None else "inf+Q" if x is None else "P+inf"
            elif x == y:
                kind = "P+P"
            elif self.r is not None and (x + y) % self.r == 0:
                kind = "P-P"
            else:
                kind = "P+Q"
            self._note(kind, phase)
        if y is None:
            return x
        if x is None:
            return y
        return self.norm(x + y)

    def dbl(self, x, phase=None):
        self._note("dbl_inf" if x is None else "dbl", phase)
        return None if x is None else self.norm(2 * x)


Z = Group()


def add(x, y):
    return Z.add(x, y)


def dbl(x):
    return Z.dbl(x)


def val(x):
    return 0 if x is None else x


def serial(L, B, stored, grp=Z, kernel="serial"):
    """k_reduce_serial / k_reduce_serial_q: one thread (quad) walks its L buckets from the last to the first; B[j] is the
    bucket's sum (None: infinity), stored[j] whether the reduction reads the record at all (an empty bucket was never
    written; slots past the last bucket are not stored either). Returns (S, W) = (sum B_j, sum (j + 1) B_j)."""
    run = tot = None
    for j in reversed(range(L)):
        grp.at(kernel, "run", j)
        if j < len(B) and stored[j]:
            run = grp.add(run, B[j])
        grp.at(kernel, "tot", j)
        tot = grp.add(tot, run)
    return run, tot


def combine_q(N, log2L, prescale, S, W, grp=Z, kernel="combine1"):
    """k_combine_q<U, INL, N>: quad j holds pair j."""
    S, W = list(S), list(W)
    lg = N.bit_length() - 1
    for s in range(lg):  # suffix scan, in place
        d = 1 << s
        grp.at(kernel, "scan", s)
        loaded = [(j, S[j], S[j + d]) for j in range(N) if j + d < N]      # quad_add_load of every active quad
        for j, x, y in loaded:                                               # after the barrier
            S[j] = grp.add(x, y)
    park = S[0]
    S[0] = None
    dbl_left = prescale
    n_tree, n_fin = lg, log2L + 1
    for s in range(n_tree + n_fin):
        loaded, fin_dbl = [], False
        grp.at(kernel, "tree" if s < n_tree else "finish", s)
        for j in range(N):
            upper = j >= N // 2
            jj = j - N // 2 if upper else j
            arr = W if upper else S
            if s < n_tree:
                d = N >> (s + 1)
                if d >= 1 and jj < d:
                    loaded.append((arr, jj, arr[jj], arr[jj + d]))
            elif j == 0:
                step = s - n_tree
                if step < log2L:
                    fin_dbl = True
                else:
                    loaded.append((W, 0, W[0], S[0]))
            if j == N - 1 and s == 0:
                assert upper and jj < (N >> 1), "quad N-1 is busy in the first tree step"
        for arr, jj, x, y in loaded:
            arr[jj] = grp.add(x, y)
        if fin_dbl:
            S[0] = grp.dbl(S[0], "lu")
        if s >= 1 and dbl_left > 0:  # the doubler (quad N-1)
            jj = N // 2 - 1
            assert s >= n_tree or jj >= (N >> (s + 1)), "the doubler must be free"
            park = grp.dbl(park, "park")
            dbl_left -= 1
    assert dbl_left == 0
    return park, W[0]


def combine_we(log2L, prescale, S, W, grp=Z, kernel="combine1"):
    """k_combine_we (N = 64): work-efficient form - pair sums per index bit, the odd elements' trees in place, then
    U = sum_l 2^l M_l by three two-term pairs. Same result as combine_q with 3.4 instead of 8 additions per pair."""
    N = 64
    S, W = list(S), list(W)
    for s in range(1, 7):
        g = 32 >> (s - 1)
        loaded = []
        grp.at(kernel, "pairs", s)
        for q in range(N):
            G, i = q // g, q % g
            if G > s:
                continue
            if G == 0:
                l = s - 1
                loaded.append((S, (2 * i) << l, S[(2 * i) << l], S[(2 * i + 1) << l]))
            elif G < s:
                l = G - 1
                loaded.append((S, (2 * i + 1) << l, S[(2 * i + 1) << l], S[(2 * (i + g) + 1) << l]))
            else:
                loaded.append((W, i, W[i], W[i + g]))
        assert len(loaded) == (s + 1) * g <= N
        dests = [(id(arr), k) for arr, k, _, _ in loaded]
        assert len(set(dests)) == len(dests), "two tasks write one record"
        for arr, k, x, y in loaded:
            arr[k] = grp.add(x, y)
    park = S[0]
    dbl_left = prescale
    m = lambda l: 1 << l  # slot of M_l
    tail = [  # (doublings, additions) of each tail step on the slots S[1], S[2], S[4], S[8], S[16], S[32]
        ([m(1), m(3), m(5)], []),
        ([], [(m(0), m(1)), (m(2), m(3)), (m(4), m(5))]),
        ([m(2), m(4)], []),
        ([m(2), m(4)], []),
        ([m(4)], [(m(0), m(2))]),
        ([m(4)], []),
        ([], [(m(0), m(4))]),
    ]
    tail += [([m(0)], [])] * log2L
    for step, (dbls, adds) in enumerate(tail + [([], [])]):
        last = (dbls, adds) == ([], [])
        grp.at(kernel, "finish" if last else "lu" if step >= 7 else "tail", step)
        loaded = [(x, S[x], S[y]) for x, y in adds]
        assert not (set(dbls) & {x for x, _ in adds}) and not (set(dbls) & {y for _, y in adds})
        for x, vx, vy in loaded:
            S[x] = grp.add(vx, vy)
        for x in dbls:
            S[x] = grp.dbl(S[x])
        if last:
            W[0] = grp.add(W[0], S[1])
        if dbl_left > 0:
            park = grp.dbl(park, "park")
            dbl_left -= 1
    assert dbl_left == 0, "the prescaling doublings must fit into the tail"
    return park, W[0]


def reduce2_q(active, nblocks1, log2span, S, W, grp=Z, kernel="reduce2"):
    """k_reduce2_q: quad j holds level-1 block j (j < nblocks1, the rest infinity)."""
    S = [S[j] if j < nblocks1 else None for j in range(active)]
    W = [W[j] if j < nblocks1 else None for j in range(active)]
    d, s = 1, 0
    while d < active:
        grp.at(kernel, "scan", s)
        loaded = [(j, S[j], S[j + d]) for j in range(active) if j + d < active]
        for j, x, y in loaded:
            S[j] = grp.add(x, y)
        d <<= 1
        s += 1
    S[0] = None
    for s in range(log2span):
        grp.at(kernel, "span", s)
        S = [grp.dbl(x) for x in S]
    grp.at(kernel, "finish", 0)
    W = [grp.add(W[j], S[j]) for j in range(active)]
    d, s = active >> 1, 0
    while d >= 1:
        grp.at(kernel, "tree", s)
        loaded = [(j, W[j], W[j + d]) for j in range(d)]
        for j, x, y in loaded:
            W[j] = grp.add(x, y)
        d >>= 1
        s += 1
    return W[0]


def reduce2_active(nlast):
    active = 2
    while active < nlast:
        active <<= 1
    return active


def reduce_window(grp, B, stored, log2L, three, we):
    """Pipeline::enqueue_reduce_kernels for one bucket set: the serial level with L = 2^log2L, one combine (two with `three`),
    k_reduce2_q. B[j]: bucket sums in grp (None = infinity), stored[j]: the record exists. Returns (total, info) with
    info = dict(S=[S_t], W=[W_t]) of the serial level."""
    NB, L, N = len(B), 1 << log2L, COMBINE_N
    T = (NB + L - 1) >> log2L
    pairs = [serial(L, B[g * L:(g + 1) * L], stored[g * L:(g + 1) * L], grp) for g in range(T)]
    info = {"S": [p[0] for p in pairs], "W": [p[1] for p in pairs]}

    def combine(pairs, l2, pre, kernel):
        out = []
        for blk in range((len(pairs) + N - 1) // N):
            part = pairs[blk * N:(blk + 1) * N] + [(None, None)] * N
            S, W = [p[0] for p in part[:N]], [p[1] for p in part[:N]]
            out.append(combine_we(l2, pre, S, W, grp, kernel) if we else combine_q(N, l2, pre, S, W, grp, kernel))
        return out

    log2span = log2L + N.bit_length() - 1
    level = combine(pairs, log2L, log2span, "combine1")
    rest = 0  # level 1 prescales by the whole span
    if three:
        assert len(level) > 1
        level = combine(level, 0, N.bit_length() - 1, "combine2")
    assert len(level) <= RED2_TPB
    total = reduce2_q(reduce2_active(len(level)), len(level), rest, [p[0] for p in level], [p[1] for p in level], grp)
    return total, info
