"""Python big-int models of the point updates of the SRS ceremony (ecc/<curve>/mpcsetup/mpcsetup.go), over oracle/pyref.py's
Group (affine points, None = infinity), shared by tests/test_mpcsetup_model.py (no GPU, no library):

  reference_update_monomials        UpdateMonomialsG1 as written (mpcsetup.go:366-381): the running power, A[0] untouched
  reference_linear_combinations     linearCombinationsG1/G2's own route (mpcsetup.go:396-447): the special case of one
                                    slice of length 2, zeros at the segment-last powers, one MSM for `truncated`, then
                                    `shifted` = r^-1 truncated corrected by 2 len(ends) head and tail terms - an MSM of
                                    2 len(ends) + 1 terms
  direct_linear_combinations        the definition gmsm_linear_combinations implements: truncated = sum r^i A[i] and
                                    shifted = sum r^i A[i + 1] over every i that is not the last of its segment

The two agree on points of the r-torsion, where r^-1 (r P) = P. The reference takes r from powers[1] AFTER zeroing the
segment-last powers and builds the correction terms in place; with ends[0] == 2 and more than one segment powers[1] is one of
the zeroed entries (and the in-place writes overtake their reads), so there its arithmetic no longer follows the comment
above it. The model keeps r and the original vectors - the route the reference's comment states - which is the same
computation wherever the first slice is longer than 2 or alone."""


def powers_of(r, n, mod):
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * r % mod
    return out


def reference_update_monomials(g, A, r):
    mod = g.c.r
    A = list(A)
    A[1] = g.mul(r % mod, A[1])
    r_exp = r * r % mod
    for i in range(2, len(A)):
        k = r_exp
        if i + 1 != len(A):
            r_exp = r_exp * r % mod
        A[i] = g.mul(k, A[i])
    return A


def check_ends(n, ends):
    prev = 0
    for e in ends:
        if e - prev < 2:
            raise ValueError("each slice must be of length at least 2")
        prev = e
    if prev != n:
        raise ValueError("lengths mismatch")


def reference_linear_combinations(g, A, r, ends):
    mod = g.c.r
    check_ends(len(A), ends)
    if len(ends) == 1 and ends[0] == 2:
        return A[0], A[1]
    powers = powers_of(r, len(A), mod)
    for e in ends:
        powers[e - 1] = 0
    truncated = g.msm(A, powers)
    r_inv_neg = -pow(r, -1, mod) % mod
    pts, sc, prev = [], [], 0
    for e in ends:
        pts += [A[prev], A[e - 1]]
        sc += [powers[prev] * r_inv_neg % mod, powers[e - 2]]
        prev = e
    pts.append(truncated)
    sc.append(-r_inv_neg % mod)
    return truncated, g.msm(pts, sc)


def direct_linear_combinations(g, A, r, ends):
    mod = g.c.r
    check_ends(len(A), ends)
    last = {e - 1 for e in ends}
    idx = [i for i in range(len(A)) if i not in last]
    pw = powers_of(r, len(A), mod)
    return g.msm([A[i] for i in idx], [pw[i] for i in idx]), g.msm([A[i + 1] for i in idx], [pw[i] for i in idx])
