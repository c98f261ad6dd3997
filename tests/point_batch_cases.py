"""Inputs for the tests of the point-batch kernels past the sizes the older suites stop at - k_fixed_base at every table width,
k_batch_normalize with whole groups at infinity, the GLV walk's table selection, Group::batch_scale beyond one chunk - and the
launch shape of the sumcheck round: tests/test_point_batch_cases.py shows on the host that every case has the property it is
named for, tests/test_gpu_point_batches.py and tests/test_gpu_gkr.py run them on the device.

The constants the cases are built round are restated here with the line each comes from; test_point_batch_cases.py reads them
back out of the sources, so that a change there fails on the host and names the test sizes that have to move with it.

borrow_cases(curve, c)        scalars with a prescribed digit in every window of width c (the model is frontend_cases.recode, which
                              is pinned to the reference's partitionScalars): the digits are written down here in closed form,
                              not taken from the model
glv_pattern_cases(curve)      (k1, k2, s = k1 + k2 lambda mod r) whose halves make the walk read one table entry only, or have a
                              given sign mix - as far as GlvParams.split, which the device's split is tied to, returns such pairs;
                              with the scalars next to the corners of the split's lattice cell, where a half changes sign
infinity_masks(n)             which records of a batch are at infinity, by the K-record groups of k_batch_normalize
round_lanes / round_workgroups  the launch shape of k_gkr_round as GkrField::gkr_new and ::round choose it"""
import importlib
import random
import warnings

import frontend_cases as fc

SCALE_CHUNK = 1 << 18    # gmsm_scale.h: static constexpr size_t SCALE_CHUNK = (size_t)1 << 18;
NORMALIZE_K = 32         # gmsm_group.h, normalize_records: constexpr int K = 32;
NORMALIZE_TPB = 64       # ... dim3(64): records [2048 j, 2048 (j + 1)) belong to workgroup j
EXPR_TPB = 256           # gmsm_iop_expr.h: constexpr unsigned EXPR_TPB = 256; (GKR_TPB = EXPR_TPB, gmsm_gkr.h)
EXPR_LDS_BYTES = 64 * 1024  # gmsm_iop_expr.h: constexpr size_t EXPR_LDS_BYTES = 64 * 1024;
FRI_TPB = 256            # gmsm_fri.h: constexpr unsigned FRI_TPB = 256;
FIXED_BASE_WIDTHS = range(2, 15)  # what GMSM_OPT_FIXED_BASE_BITS admits

# (curve, c) with c | fr_bits: the top window is a full one, lastC = c + 1 and its bucket set has 2^c entries (gmsm_context.h, last_c)
EXACTLY_DIVIDING = [("bn254", 2), ("bls12_381", 3), ("bls12_381", 5), ("bw6_761", 13)]

# the widths tests/test_gpu_point_batches.py runs the fixed-base batch at
FIXED_BASE_CASES = ([("bn254", "g1", c) for c in FIXED_BASE_WIDTHS]
                    + [("bn254", "g2", 2), ("bn254", "g2", 13)]
                    + [("bls12_381", "g1", 3), ("bls12_381", "g1", 5), ("bls12_381", "g1", 13)]
                    + [("bls12_381", "g2", 5), ("bls12_381", "g2", 11)]
                    + [("bw6_761", "g1", 13), ("bw6_761", "g1", 14)]
                    + [("bw6_761", "g2", 8), ("bw6_761", "g2", 13)])


class CaseCannotBeBuilt(ValueError):
    """a prescribed pattern does not exist for this curve and width"""


def _curve(curve):
    """a curve object (.name, .r, .fr_bits) as it is, or the one of a name"""
    return importlib.import_module("gnark-crypto_amd").curves.CURVES[curve] if isinstance(curve, str) else curve


# ------------------------------------------------------------------ fixed base: digits and borrows
def _from_raw(curve, raw, c):
    """the scalar whose unsigned c-bit windows are `raw`"""
    s = sum(u << (c * w) for w, u in enumerate(raw))
    if not (all(0 <= u < 1 << c for u in raw) and s < curve.r):
        raise CaseCannotBeBuilt((curve.name, c, raw))
    return s


def borrow_cases(curve, c):
    """[(name, scalar, digits or None)]: digits[w] is the signed digit partitionScalars must give window w (a negative one has
    borrowed 2^c from window w + 1), None where only the value is prescribed (r - 1, r - 2). curve: a curve object or its name"""
    curve = _curve(curve)
    bits = curve.fr_bits
    nwin, half, ones = fc.num_windows(bits, c), 1 << (c - 1), (1 << c) - 1
    low = nwin - 1                              # windows below the top
    top_max = (curve.r - 1) >> (c * low)        # the top window of the largest scalar
    if nwin < 3 or top_max < 1:
        raise CaseCannotBeBuilt((curve.name, c))
    top = top_max - 1                           # any lower windows stay below r
    out = []

    def add(name, raw, digits):
        assert len(raw) == len(digits) == nwin
        out.append((name, _from_raw(curve, raw, c), list(digits)))

    # every window at 2^(c-1): the first borrows, and its carry makes every later one 2^(c-1) + 1, which borrows again
    add("all_half", [half] * low + [top], [-half] + [-(half - 1)] * (low - 1) + [top + 1])
    # every window at 2^(c-1) - 1: the largest digit that stays
    add("all_half_minus_one", [half - 1] * low + [top], [half - 1] * low + [top])
    # all ones / zero in turn: -1 with a borrow, then 0 + 1
    add("ones_zero", [ones if w % 2 == 0 else 0 for w in range(low)] + [top],
        [-1 if w % 2 == 0 else 1 for w in range(low)] + [top + (1 if low % 2 == 1 else 0)])
    add("zero_ones", [0 if w % 2 == 0 else ones for w in range(low)] + [top],
        [(0 if w == 0 else 1) if w % 2 == 0 else -1 for w in range(low)] + [top + (1 if low % 2 == 0 else 0)])
    # 2^(c-1) / zero in turn: the smallest digit that borrows, its carry alone in the next window
    add("half_zero", [half if w % 2 == 0 else 0 for w in range(low)] + [top],
        [-half if w % 2 == 0 else 1 for w in range(low)] + [top + (1 if low % 2 == 1 else 0)])
    out.append(("r_minus_1", curve.r - 1, None))
    out.append(("r_minus_2", curve.r - 2, None))
    # window boundaries on a 32-bit word edge of the scalar and one bit to either side of it
    edges = [j for j in range(1, nwin) if (c * j) % 32 in (31, 0, 1)]
    if not edges:
        raise CaseCannotBeBuilt((curve.name, c, "no window boundary at a word edge"))
    for j in edges:
        # j windows of ones: -1, then 2^c - 1 + 1 borrows and leaves the digit 0, the carry lands in window j
        add("below_2^%d" % (c * j), [ones] * j + [0] * (nwin - j), [-1] + [0] * (j - 1) + [1] + [0] * (nwin - 1 - j))
        add("2^%d" % (c * j), [0] * j + [1] + [0] * (nwin - 1 - j), [0] * j + [1] + [0] * (nwin - 1 - j))
    # the largest top window of a scalar below r, alone (all_half reaches the same digit as top_max - 1 plus a carry)
    add("top_max", [0] * low + [top_max], [0] * low + [top_max])
    return out


def borrow_scalars(curve, c):
    return [s for _, s, _ in borrow_cases(curve, c)]


def word_edges(curve, c):
    """(j, c j mod 32) of the window boundaries borrow_cases() puts a power of two at"""
    curve = _curve(curve)
    return [(j, (c * j) % 32) for j in range(1, fc.num_windows(curve.fr_bits, c)) if (c * j) % 32 in (31, 0, 1)]


# ------------------------------------------------------------------ the GLV walk: which table entries a scalar reads
GLV_DIRECTIONS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]


def glv_kind(k1, k2):
    """what the joint walk of gmsm_walk.h reads for the halves (k1, k2): T[1] = +-P, T[2] = +-phi(P), T[3] their sum"""
    if k1 == 0 and k2 == 0:
        return "none"
    if k2 == 0:
        return "only_T1"
    if k1 == 0:
        return "only_T2"
    if abs(k1) == abs(k2):
        return "only_T3"
    return "mixed"


def glv_signs(k1, k2):
    return ("-" if k1 < 0 else "+") + ("-" if k2 < 0 else "+")


_glv_cache = {}


def glv_edge_scalars(curve, lam):
    """scalars whose halves lie next to the corners and edges of the cell the split reduces into: a + b lambda mod r for small
    a, b (r - 1, r - lambda and 1 - lambda among them) - where a half that is positive in the cell's interior dips below zero"""
    return sorted({(a + b * lam) % curve.r for a in range(-2, 3) for b in range(-2, 3)} - {0})


def glv_pattern_cases(curve):
    """[(name, k1, k2, s)] with GlvParams(curve).split(s) == (k1, k2); curve: a curve object or its name. For every direction d
    of GLV_DIRECTIONS the candidates are t d for t = 1, every power of two below 2^bits and a random t of every length; kept are
    the unit pair, the longest power of two and the longest random t that the split returns as they are (it reduces s into ONE
    cell of the lattice, so most candidates come back as another representative: those are dropped, with a warning that counts
    them). Added are r - 1, r - lambda, 1 - lambda and every further scalar of glv_edge_scalars() whose halves have a kind or a
    sign mix not met so far, and a random scalar of every sign mix that 2000 uniform scalars show."""
    curve = _curve(curve)
    if curve.name in _glv_cache:
        return _glv_cache[curve.name]
    glv = importlib.import_module("gnark-crypto_amd").curves.GlvParams(curve)
    rng = random.Random("glv-patterns/" + curve.name)
    r, lam, bits = curve.r, glv.lam, glv.bits
    out, dropped, empty = [], 0, []
    for d in GLV_DIRECTIONS:
        unit = pow2 = rnd = None
        for length in range(1, bits + 1):
            for which, t in (("pow2", 1 << (length - 1)), ("rnd", rng.getrandbits(length) | 1 << (length - 1))):
                k1, k2 = d[0] * t, d[1] * t
                s = (k1 + k2 * lam) % r
                if glv.split(s) != (k1, k2):
                    dropped += 1
                    continue
                if t == 1:
                    unit = (k1, k2, s)
                if which == "pow2":
                    pow2 = (k1, k2, s)
                else:
                    rnd = (k1, k2, s)
        found = [(tag, v) for tag, v in (("unit", unit), ("pow2", pow2), ("random", rnd)) if v is not None]
        if not found:
            empty.append(d)
        seen = set()
        for tag, v in found:
            if v not in seen:
                seen.add(v)
                out.append(("%s%+d%+d" % (tag, d[0], d[1]),) + v)
    met = {(glv_kind(k1, k2), glv_signs(k1, k2)) for _, k1, k2, _ in out}
    always = {"r-1": r - 1, "r-lambda": r - lam, "1-lambda": (1 - lam) % r}
    for name, s in list(always.items()) + [("edge%d" % i, s) for i, s in enumerate(glv_edge_scalars(curve, lam))]:
        k1, k2 = glv.split(s)
        key = (glv_kind(k1, k2), glv_signs(k1, k2))
        if name in always or key not in met:
            met.add(key)
            out.append((name, k1, k2, s))
    mixes = {}
    for _ in range(2000):
        s = rng.randrange(r)
        k1, k2 = glv.split(s)
        if glv_kind(k1, k2) == "mixed":
            mixes.setdefault(glv_signs(k1, k2), (k1, k2, s))
    for sg in sorted(mixes):
        out.append(("mix" + sg,) + mixes[sg])
    warnings.warn("%s: the split returned another representative for %d candidate pairs; no pair at all along %s"
                  % (curve.name, dropped, empty or "no direction"))
    _glv_cache[curve.name] = out
    return out


def glv_pattern_scalars(curve):
    return [s for _, _, _, s in glv_pattern_cases(curve)]


# What the halves of each curve's split can be: kind -> sign mixes. The split floors m1 and m2, so (k1, k2) = e1 A1 + e2 A2 with
# A1 = (a11, a12), A2 = (a21, a22) and e1, e2 in [0, 1 + 2^-32) (GlvParams: the rounding of b1, b2 costs less than 2^-32). a11 and
# a21 are positive on all three curves (asserted by test_point_batch_cases.py), so k1 >= 0 always and k1 = 0 only for s = 0: the
# walk's `neg & 1` branch and a walk over T[2] alone cannot be reached through an entry that takes a scalar. The sign of k2 is
# that of a12 or a22 in the interior of the cell; the 2^-32 of slack lets a half dip past zero next to an edge, which is how
# BLS12-381, with A2 = (128 bits, -1), gives k2 = -1 for r - 1 and k2 = -2 for r - lambda. Beyond the argument the table is what
# glv_pattern_cases() finds along the eight directions, next to the cell's corners and in uniform scalars; the host test holds it
# against that search in both directions, and the device tests run whatever the search returns.
GLV_REACHABLE = {
    "bn254": {"only_T1": {"++"}, "only_T3": {"+-"}, "mixed": {"+-"}},
    "bls12_381": {"only_T1": {"++"}, "only_T3": {"++"}, "mixed": {"++", "+-"}},
    "bw6_761": {"only_T1": {"++"}, "only_T3": {"++"}, "mixed": {"++", "+-"}},
}


# ------------------------------------------------------------------ normalisation: whole groups at infinity
GROUP_PATTERNS = ("whole", "first", "last", "all_but_one", "none", "ends")


def _group_mask(pattern, size):
    if pattern == "whole":
        return [True] * size
    if pattern == "none":
        return [False] * size
    if pattern == "first":
        return [i == 0 for i in range(size)]
    if pattern == "last":
        return [i == size - 1 for i in range(size)]
    if pattern == "ends":
        return [i in (0, size - 1) for i in range(size)]
    assert pattern == "all_but_one"
    return [i != min(7, size - 1) for i in range(size)]


def infinity_masks(n, K=NORMALIZE_K):
    """[(name, mask)]: mask[i] says record i is at infinity. The groups of K records (one thread of k_batch_normalize each) are
    independent, so one batch holds a different pattern in every group: shift j gives group g the pattern (g + j) mod 6, and the
    six shifts give every group every pattern - group 0, group 1 = [32, 64) and the cut last group among them. Then the whole
    batch."""
    out = []
    for shift in range(len(GROUP_PATTERNS)):
        mask = []
        for g in range((n + K - 1) // K):
            mask += _group_mask(GROUP_PATTERNS[(g + shift) % len(GROUP_PATTERNS)], min(K, n - g * K))
        out.append(("shift%d" % shift, mask))
    out.append(("whole_batch", [True] * n))
    return out


NORMALIZE_SIZES = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049]
NORMALIZE_SIZES_WIDE = [1, 31, 32, 33, 63, 64, 65, 2049]  # BW6-761 and the G2 groups


# ------------------------------------------------------------------ the sumcheck round's launch shape
def expr_lanes_for(elem_bytes, rows):
    """gmsm_iop_expr.h, expr_lanes_for<Fr>(rows)"""
    lanes = EXPR_TPB
    while lanes > 64 and rows * elem_bytes * lanes > EXPR_LDS_BYTES:
        lanes >>= 1
    return lanes


def round_lanes(elem_bytes, nregs, half):
    """the workgroup of k_gkr_round for a round over `half` lanes: c.lanes = expr_lanes_for(nregs + 1) (GkrField::gkr_new), then
    the shrink loop of GkrField::round"""
    lanes = expr_lanes_for(elem_bytes, nregs + 1)
    while lanes > 64 and lanes // 2 >= half:
        lanes >>= 1
    return lanes


def round_workgroups(elem_bytes, nregs, n):
    """workgroups of every round of a claim over 2^n instances: the first round and the n - 1 folds"""
    out = []
    for j in range(n):
        half = 1 << (n - 1 - j)
        out.append((half + round_lanes(elem_bytes, nregs, half) - 1) // round_lanes(elem_bytes, nregs, half))
    return out


# ------------------------------------------------------------------ the sumcheck claims of 512 workgroups
def pairs8(*x):
    """a gate of 8 inputs and degree 2: t_j = x_j + x_(j+1 mod 8), the even sums first, so that every input is still needed when
    the odd ones are made, and the 8 sums stay live across the four products"""
    t = [None] * 8
    for j in (0, 2, 4, 6, 1, 3, 5, 7):
        t[j] = x[j] + x[(j + 1) % 8]
    r = t[0] * t[1]
    r = r + t[2] * t[3]
    r = r + t[4] * t[5]
    return r + t[6] * t[7]


# name -> (callable, inputs, declared degree) of the gates below (tests/test_gpu_gkr.py has them in its GATES)
GKR_GATES = {"pairs8": (pairs8, 8, 2), "identity": (lambda x: x, 1, 1)}

# (curve, gate, n, k, lanes of the round kernel): 2^(n-1) / lanes = 512 workgroups in the first round
MANY_WORKGROUPS = [("bw6_761", "pairs8", 16, 1, 64), ("bw6_761", "pairs8", 16, 2, 64), ("bn254", "identity", 18, 1, 256)]
