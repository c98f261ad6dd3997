"""The tiling of gmsm_poly.h restated in Python (no GPU): the three-pass suffix scan - lane Horner + log-step scan per tile,
the carry pass over the tile values, the apply pass - and its one-launch form for a single tile equal the reference's
sequential eval (kzg.go:55-63) and dividePolyByXminusA (kzg.go:565-583) for every length up to 70 and around lane and tile
boundaries, at small lane widths and lane counts, for the three scalar fields."""
import importlib
import random

import pytest

curves = importlib.import_module("gnark-crypto_amd.curves")  # tests/conftest.py puts the repository root on sys.path

MODULI = {name: curves.CURVES[name].r for name in ("bn254", "bls12_381", "bw6_761")}


# ---- the reference, sequentially
def ref_eval(p, a, r):
    res = p[-1]
    for i in range(len(p) - 2, -1, -1):
        res = (res * a + p[i]) % r
    return res


def ref_divide(p, fa, a, r):
    f = list(p)
    f[0] = (f[0] - fa) % r
    for i in range(len(f) - 2, -1, -1):
        f[i] = (f[i] + f[i + 1] * a) % r
    return f[1:]


# ---- the kernels' arithmetic (k_poly_lanes, k_poly_apply, PolyField::suffix), TPB lanes per tile, lanes of 2^tb
def lane_horner(v, m, g, tb, base, r):
    lo, hi = g << tb, min((g << tb) + (1 << tb), m)
    acc = 0
    for i in range(hi - 1, lo - 1, -1):
        acc = (acc * base + v[i]) % r
    return acc


def lane_walk(v, m, g, tb, base, y, out, shift, r):
    lo, hi = g << tb, min((g << tb) + (1 << tb), m)
    for i in range(hi, lo, -1):
        y = (y * base + v[i - 1]) % r
        if out is not None and i - 1 >= shift:
            out[i - 1 - shift] = y
    return y if lo == 0 and lo < hi else None


def tile_scan(v, m, t, tpb, log_tpb, tb, pw, b0, r):
    """k_poly_lanes of workgroup t: the lanes' Horner sums, then x_l += p[b0 + tb + j] * x_(l + 2^j) for j < log2 TPB"""
    x = [lane_horner(v, m, t * tpb + l, tb, pw[b0], r) for l in range(tpb)]
    for j in range(log_tpb):
        d = 1 << j
        x = [(x[l] + (pw[b0 + tb + j] * x[l + d] if l + d < tpb else 0)) % r for l in range(tpb)]
    return x


def fused(v, m, tpb, log_tpb, tb, pw, b0, out, shift, r):
    x = tile_scan(v, m, 0, tpb, log_tpb, tb, pw, b0, r)
    value = None
    for l in range(tpb):
        y = lane_walk(v, m, l, tb, pw[b0], x[l + 1] if l + 1 < tpb else 0, out, shift, r)
        value = y if y is not None else value
    return value


def suffix(f, a, r, log_tpb, tb):
    """(h, f(a)) the way PolyField::suffix computes them"""
    m, tpb = len(f), 1 << log_tpb
    pw = [pow(a, 1 << b, r) for b in range(40)]  # FftPowers
    logL = log_tpb + tb
    L = 1 << logL
    nt = (m + L - 1) // L
    h = [None] * (m - 1)
    if nt <= 1:
        value = fused(f, m, tpb, log_tpb, tb, pw, 0, h, 1, r)
        return h, value
    X, S = [], []
    for t in range(nt):  # pass 1
        x = tile_scan(f, m, t, tpb, log_tpb, tb, pw, 0, r)
        X += x
        S.append(x[0])
    tc = 0
    while (tpb << tc) < nt:
        tc += 1
    C = [None] * nt  # pass 2: one workgroup over the tile values, base a^L = p[logL]
    fused(S, nt, tpb, log_tpb, tc, pw, logL, C, 0, r)
    apow = [pow(a, (1 << tb) * k, r) for k in range(tpb)]  # k_fft_pow_table over the powers of a^T
    value = None
    for t in range(nt):  # pass 3
        for l in range(tpb):
            g = t * tpb + l
            cin = X[g + 1] if l + 1 < tpb else 0
            if t + 1 < nt:
                cin = (cin + apow[tpb - 1 - l] * C[t + 1]) % r
            y = lane_walk(f, m, g, tb, pw[0], cin, h, 1, r)
            value = y if y is not None else value
    return h, value


def eval_only(f, a, r, log_tpb, tb):
    """passes 1-2 only (gmsm_poly_eval): f(a) = C_0"""
    m, tpb = len(f), 1 << log_tpb
    pw = [pow(a, 1 << b, r) for b in range(40)]
    logL = log_tpb + tb
    nt = (m + (1 << logL) - 1) >> logL
    if nt <= 1:
        return fused(f, m, tpb, log_tpb, tb, pw, 0, None, 1, r)
    S = [tile_scan(f, m, t, tpb, log_tpb, tb, pw, 0, r)[0] for t in range(nt)]
    tc = 0
    while (tpb << tc) < nt:
        tc += 1
    return fused(S, nt, tpb, log_tpb, tc, pw, logL, [None] * nt, 0, r)


def points(r, rnd):
    return [0, 1, r - 1, rnd.randrange(r)]


# (log2 lanes per tile, log2 coefficients per lane): one tile = 4..32 coefficients, so 1..70 crosses many tiles
SHAPES = [(1, 1), (2, 1), (2, 2), (3, 2)]


@pytest.mark.parametrize("curve", sorted(MODULI))
@pytest.mark.parametrize("shape", SHAPES)
def test_tiled_suffix_equals_reference(curve, shape):
    r = MODULI[curve]
    log_tpb, tb = shape
    rnd = random.Random(f"{curve}/{shape}")
    for n in range(1, 71):
        f = [rnd.randrange(r) for _ in range(n)]
        for a in points(r, rnd):
            fa = ref_eval(f, a, r)
            h, value = suffix(f, a, r, log_tpb, tb)
            assert value == fa, (n, a)
            assert h == ref_divide(f, fa, a, r), (n, a)
            assert eval_only(f, a, r, log_tpb, tb) == fa, (n, a)


@pytest.mark.parametrize("curve", sorted(MODULI))
def test_tile_and_lane_boundaries(curve):
    """lengths one below, at and one above a lane, a tile and several tiles, with many tiles per carry lane"""
    r = MODULI[curve]
    rnd = random.Random(curve)
    log_tpb, tb = 2, 2
    lane, tile = 1 << tb, 1 << (log_tpb + tb)
    lengths = sorted({x + d for x in (lane, tile, 2 * tile, 5 * tile, tile * tile // lane, 4 * tile * (1 << log_tpb)) for d in (-1, 0, 1)})
    for n in lengths:
        f = [rnd.randrange(r) for _ in range(n)]
        a = rnd.randrange(r)
        fa = ref_eval(f, a, r)
        h, value = suffix(f, a, r, log_tpb, tb)
        assert (value, h) == (fa, ref_divide(f, fa, a, r)), n


@pytest.mark.parametrize("curve", sorted(MODULI))
def test_quotient_identity(curve):
    """h (X - a) + f(a) = f coefficient by coefficient"""
    r = MODULI[curve]
    rnd = random.Random(curve + "/identity")
    for n in (1, 2, 3, 17, 33, 70):
        f = [rnd.randrange(r) for _ in range(n)]
        for a in points(r, rnd):
            h, value = suffix(f, a, r, 2, 1)
            prod = [0] * n  # h (X - a)
            for k, hk in enumerate(h):
                prod[k + 1] = (prod[k + 1] + hk) % r
                prod[k] = (prod[k] - a * hk) % r
            prod[0] = (prod[0] + value) % r
            assert prod == f, (n, a)


def test_fold_model():
    """F_j = sum_i gamma^i f_(i,j), f_(i,j) = 0 beyond len(f_i), as k_poly_fold computes it (Horner in gamma) and as
    BatchOpenSinglePoint's loop does (kzg.go:302-320)"""
    r = MODULI["bn254"]
    rnd = random.Random("fold")
    polys = [[rnd.randrange(r) for _ in range(n)] for n in (5, 1, 9, 3)]
    gamma = rnd.randrange(r)
    maxlen = max(map(len, polys))
    ref = list(polys[0]) + [0] * (maxlen - len(polys[0]))
    g = gamma
    for p in polys[1:]:
        for j, c in enumerate(p):
            ref[j] = (ref[j] + g * c) % r
        g = g * gamma % r
    horner = []
    for j in range(maxlen):
        acc = 0
        for p in reversed(polys):
            acc = (acc * gamma + (p[j] if j < len(p) else 0)) % r
        horner.append(acc)
    assert horner == ref
