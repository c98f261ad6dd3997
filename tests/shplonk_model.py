"""Two Python big-int models of shplonk.BatchOpen (ecc/<curve>/shplonk/shplonk.go:44-172) over integers mod r, shared by
tests/test_shplonk_model.py and tests/test_gpu_shplonk.py (no GPU, no library):

  reference_batch_open   the reference AS WRITTEN: buildZtMinusSi, interpolate through buildLagrangeFromDomain, the naive
                         mul by Z_(T\\S_i), the naive div by Z_T, the assembly of L with its padding to totalSize and the
                         naive div by (X - z) - helper for helper, buffer for buffer
  chain_batch_open       the formulation gmsm_shplonk.h runs: per polynomial a chain of divisions by (X - s), whose
                         remainders are the Newton coefficients of r_i; w = sum_i gamma^i q_i; claimed values and r_i(z)
                         from the Newton form; L in one pass and one division by (X - z)

Polynomials are lists of ints (true values, lowest degree first), points a list of lists, gamma and z ints."""


# ---- the reference's helpers (shplonk.go:313-464), in its own words
def flatten(x):
    return [p for s in x for p in s]


def eval_poly(f, x, r):
    y = 0
    for c in reversed(f):
        y = (y * x + c) % r
    return y


def mul_by_constant(f, c, r):
    for i in range(len(f)):
        f[i] = f[i] * c % r
    return f


def multiply_linear_factor(f, a, r):
    s = len(f)
    f = f + [0]
    f[s] = f[s - 1]
    for i in range(s - 1, 0, -1):
        f[i] = (f[i - 1] - f[i] * a) % r
    f[0] = -(f[0] * a) % r
    return f


def build_vanishing_poly(x, r):
    res = [1]
    for a in x:
        res = multiply_linear_factor(res, a, r)
    return res


def build_zt_minus_si(x, i, r):
    return build_vanishing_poly(flatten(x[:i]) + flatten(x[i + 1:]), r)


def build_lagrange_from_domain(x, i, r):
    res = build_vanishing_poly(x[:i] + x[i + 1:], r)
    d = pow(eval_poly(res, x[i], r), -1, r)
    return mul_by_constant(res, d, r)


def interpolate(x, y, r):
    res = [0] * len(x)
    for i in range(len(x)):
        li = mul_by_constant(build_lagrange_from_domain(x, i, r), y[i], r)
        for j in range(len(x)):
            res[j] = (res[j] + li[j]) % r
    return res


def mul(f, g, res, r):
    size_res = len(f) + len(g) - 1
    if len(res) < size_res:
        res = res + [0] * (size_res - len(res))
    for i in range(len(res)):
        res[i] = 0
    for i in range(len(g)):
        for j in range(len(f)):
            res[j + i] = (res[j + i] + f[j] * g[i]) % r
    return res


def div(f, g, r):
    sizef, sizeg = len(f), len(g)
    for i in range(sizef - 2, sizeg - 2, -1):
        for j in range(sizeg - 1):
            f[i - j] = (f[i - j] - f[i + 1] * g[sizeg - 2 - j]) % r
    return f[sizeg - 1:]


def reference_batch_open(polynomials, points, gamma, z, r):
    """(w, claimed, wprime) as shplonk.go:66-164 computes them: w has maxSizePolys coefficients, wprime totalSize - 1."""
    nb = len(polynomials)
    max_size = max(len(p) for p in polynomials)
    for s in points:
        max_size = max(max_size, len(s) + 1)
    nb_points = sum(len(s) for s in points)
    total = max_size + nb_points
    buf_max = [0] * max_size
    buf_total = [0] * total
    f = [0] * total
    claimed = [[eval_poly(polynomials[i], s, r) for s in points[i]] for i in range(nb)]
    acc = 1
    zt_minus_si, ri = [], []
    for i in range(nb):
        zt_minus_si.append(build_zt_minus_si(points, i, r))
        buf_max[:len(polynomials[i])] = polynomials[i]
        ri.append(interpolate(points[i], claimed[i], r))
        for j in range(len(ri[i])):
            buf_max[j] = (buf_max[j] - ri[i][j]) % r
        buf_total = mul(buf_max, zt_minus_si[i], buf_total, r)
        buf_total = mul_by_constant(buf_total, acc, r)
        for j in range(len(buf_total)):
            f[j] = (f[j] + buf_total[j]) % r
        acc = acc * gamma % r
        buf_max = [0] * max_size
    zt = build_vanishing_poly(flatten(points), r)
    w = div(f, zt, r)
    # second half, after z
    acc = 1
    big_l = [0] * total
    for i in range(nb):
        c = acc * eval_poly(zt_minus_si[i], z, r) % r
        buf_max[:len(polynomials[i])] = polynomials[i]
        buf_max[0] = (buf_max[0] - eval_poly(ri[i], z, r)) % r
        for j in range(len(polynomials[i])):
            buf_max[j] = buf_max[j] * c % r
        for j in range(len(buf_max)):
            big_l[j] = (big_l[j] + buf_max[j]) % r
        buf_max = [0] * max_size
        acc = acc * gamma % r
    ztz = eval_poly(zt, z, r)
    buf_total = [0] * total
    buf_total[:len(w)] = w
    mul_by_constant(buf_total, ztz, r)
    for i in range(total - max_size):
        big_l[total - 1 - i] = -buf_total[total - 1 - i] % r
    for i in range(max_size):
        big_l[i] = (big_l[i] - buf_total[i]) % r
    wprime = div(big_l, build_vanishing_poly([z], r), r)
    return list(w), claimed, wprime


# ---- the chain / Newton / accumulate formulation
def divide_by_x_minus_a(f, a, r):
    """(quotient, remainder) of f by (X - a): the suffix recurrence y_i = f_i + a y_(i+1)"""
    y, ys = 0, [0] * len(f)
    for i in range(len(f) - 1, -1, -1):
        y = (f[i] + a * y) % r
        ys[i] = y
    return ys[1:], ys[0]


def newton_eval(s, d, x, r):
    acc = 0
    for j in range(len(d) - 1, -1, -1):
        acc = (acc * (x - s[j]) + d[j]) % r
    return acc


def newton_from_values(s, y, r):
    d = list(y)
    for level in range(1, len(s)):
        for j in range(len(s) - 1, level - 1, -1):
            d[j] = (d[j] - d[j - 1]) * pow(s[j] - s[j - level], -1, r) % r
    return d


def chain_open_w(polynomials, points, gamma, r):
    """(w, claimed): w has max_i len(f_i) coefficients"""
    maxlen = max(len(p) for p in polynomials)
    w = [0] * maxlen
    claimed, acc = [], 1
    for f, s in zip(polynomials, points):
        q, d = list(f), []
        for a in s:
            if not q:  # the chain ran out of coefficients: the quotient is empty and r_i = f_i
                d.append(0)
                continue
            q, rem = divide_by_x_minus_a(q, a, r)
            d.append(rem)
        for j, c in enumerate(q):
            w[j] = (w[j] + acc * c) % r
        claimed.append([newton_eval(s[:j + 1], d[:j + 1], s[j], r) for j in range(len(s))])
        acc = acc * gamma % r
    return w, claimed


def chain_open_wprime(polynomials, points, claimed, gamma, w, z, r):
    """wprime: max_i len(f_i) - 1 coefficients"""
    maxlen = max(len(p) for p in polynomials)
    zs = []
    for s in points:
        v = 1
        for a in s:
            v = v * (z - a) % r
        zs.append(v)
    ztz = 1
    for v in zs:
        ztz = ztz * v % r
    big_l = [-ztz * w[j] % r for j in range(maxlen)]
    acc = 1
    for i, (f, s) in enumerate(zip(polynomials, points)):
        c = acc
        for l, v in enumerate(zs):
            if l != i:
                c = c * v % r
        for j in range(len(f)):
            big_l[j] = (big_l[j] + c * f[j]) % r
        big_l[0] = (big_l[0] - c * newton_eval(s, newton_from_values(s, claimed[i], r), z, r)) % r
        acc = acc * gamma % r
    return divide_by_x_minus_a(big_l, z, r)[0]


def chain_batch_open(polynomials, points, gamma, z, r):
    w, claimed = chain_open_w(polynomials, points, gamma, r)
    return w, claimed, chain_open_wprime(polynomials, points, claimed, gamma, w, z, r)


def strip(p):
    p = list(p)
    while p and p[-1] == 0:
        p.pop()
    return p
