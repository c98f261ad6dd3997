"""Two Python big-int models of fflonk.BatchOpen (ecc/<curve>/fflonk/fflonk.go:41-141) over integers mod r, shared by
tests/test_fflonk_model.py and tests/test_gpu_fflonk.py (no GPU, no library):

  reference_batch_open   the reference AS WRITTEN: getNextDivisorRMinusOne, getIthRootOne, extendSet, Fold, eval at z^t,
                         then shplonk_model.reference_batch_open on the folded polynomials and the extended sets
  shortcut_batch_open    the formulation gmsm_fflonk.h runs: per member a chain of divisions by (Y - z_k^t) on the polynomial
                         as given, gamma^i times the quotient added into its residue class of w, the outer claimed values
                         from the chain's Newton remainders, the inner ones from the outer ones, L read through the pack
                         index (member e mod t, coefficient e div t) and one division by (X - z)

packs[i] is a list of polynomials (lists of ints, true values, lowest degree first; an empty list is the zero
polynomial), points[i] the base points of pack i, gamma and z ints, r the modulus, g a generator of Fr^*."""
import shplonk_model as sm


def next_divisor(i, r):
    """getNextDivisorRMinusOne (fflonk.go:234-252); None where the reference panics"""
    tmp = (r - 1) % i
    trials = 100
    while tmp != 0 and trials > 0:
        i += 1
        tmp = (r - 1) % i
        trials -= 1
    if trials == 0:
        return None
    return i


def ith_root_one(i, r, g):
    """getIthRootOne (fflonk.go:213-230)"""
    assert (r - 1) % i == 0, "fr does not contain all the t-th roots of 1"
    return pow(g, (r - 1) // i, r)


def extend_set(p, t, r, g):
    """extendSet (fflonk.go:255-271): [p0, w p0, .., w^(t-1) p0, p1, ..]"""
    omega = ith_root_one(t, r, g)
    out = [0] * (t * len(p))
    for i in range(len(p)):
        out[i * t] = p[i]
        for k in range(1, t):
            out[i * t + k] = out[i * t + k - 1] * omega % r
    return out


def fold(p, r):
    """Fold (fflonk.go:52-71)"""
    t = next_divisor(len(p), r)
    size = max(len(q) for q in p) * t
    buf = [0] * size
    for i in range(len(p)):
        for j in range(len(p[i])):
            buf[j * t + i] = p[i][j]
    return buf


def reference_batch_open(packs, points, gamma, z, r, g):
    """(w, claimed, folded_claimed, wprime): claimed[i][j][k] as OpeningProof.ClaimedValues, the rest as
    shplonk_model.reference_batch_open returns them for the folded polynomials on the extended sets"""
    assert len(packs) == len(points)
    ts = [next_divisor(len(p), r) for p in packs]
    powers = [[pow(x, t, r) for x in s] for s, t in zip(points, ts)]
    claimed = []
    for p, t, a in zip(packs, ts, powers):
        rows = [[sm.eval_poly(q, x, r) for x in a] for q in p]
        rows += [[0] * len(a) for _ in range(len(p), t)]  # the remaining polynomials are zero
        claimed.append(rows)
    folded = [fold(p, r) for p in packs]
    new_points = [extend_set(s, t, r, g) for s, t in zip(points, ts)]
    w, folded_claimed, wprime = sm.reference_batch_open(folded, new_points, gamma, z, r)
    return w, claimed, folded_claimed, wprime


def shortcut_open_w(packs, points, gamma, r, g):
    """(w, claimed, folded_claimed): w has max_i t_i n_i coefficients"""
    ts = [next_divisor(len(p), r) for p in packs]
    wlen = max(t * max(len(q) for q in p) for p, t in zip(packs, ts))
    w = [0] * wlen
    claimed, folded_claimed, acc = [], [], 1
    for p, s, t in zip(packs, points, ts):
        a = [pow(x, t, r) for x in s]
        rows = []
        for j, f in enumerate(p):
            q, d = list(f), []
            for x in a:
                if not q:  # the chain ran out of coefficients (or the member is empty): the quotient is empty
                    d.append(0)
                    continue
                q, rem = sm.divide_by_x_minus_a(q, x, r)
                d.append(rem)
            for e, c in enumerate(q):
                w[e * t + j] = (w[e * t + j] + acc * c) % r
            rows.append([sm.newton_eval(a[:k + 1], d[:k + 1], a[k], r) for k in range(len(a))])
        ext = extend_set(s, t, r, g)
        inner = [0] * (t * len(s))
        for k in range(len(s)):
            for l in range(t):
                inner[k * t + l] = sm.eval_poly([row[k] for row in rows], ext[k * t + l], r)
        claimed.append(rows + [[0] * len(s) for _ in range(len(p), t)])
        folded_claimed.append(inner)
        acc = acc * gamma % r
    return w, claimed, folded_claimed


def shortcut_open_wprime(packs, points, folded_claimed, gamma, w, z, r, g):
    """wprime: max_i t_i n_i - 1 coefficients"""
    ts = [next_divisor(len(p), r) for p in packs]
    ext = [extend_set(s, t, r, g) for s, t in zip(points, ts)]
    zs = []
    for s in ext:
        v = 1
        for x in s:
            v = v * (z - x) % r
        zs.append(v)
    ztz = 1
    for v in zs:
        ztz = ztz * v % r
    big_l = [-ztz * c % r for c in w]
    acc = 1
    for i, (p, t) in enumerate(zip(packs, ts)):
        c = acc
        for l, v in enumerate(zs):
            if l != i:
                c = c * v % r
        for e in range(len(w)):
            j, d = e % t, e // t
            if j < len(p) and d < len(p[j]):
                big_l[e] = (big_l[e] + c * p[j][d]) % r
        big_l[0] = (big_l[0] - c * sm.newton_eval(ext[i], sm.newton_from_values(ext[i], folded_claimed[i], r), z, r)) % r
        acc = acc * gamma % r
    return sm.divide_by_x_minus_a(big_l, z, r)[0]


def shortcut_batch_open(packs, points, gamma, z, r, g):
    w, claimed, folded_claimed = shortcut_open_w(packs, points, gamma, r, g)
    return w, claimed, folded_claimed, shortcut_open_wprime(packs, points, folded_claimed, gamma, w, z, r, g)
