"""Big-int model of the reference's GKR prover and verifier: fr/polynomial.MultiLin (multilin.go), fiat-shamir/transcript.go,
fr/sumcheck/sumcheck.go and fr/gkr/gkr.go, loop for loop, over Python ints mod p. Test infrastructure: the device code is
compared against it, and it is itself pinned by the reference's eight golden proofs (tests/golden/gkr_vectors.json).

A circuit is a list of (gate name or None, [input wire indices]); an assignment a list, per wire, of 2^n values (or None
before complete()). A proof is a list, per SORTED wire, of {"partialSumPolys": [[..], ..], "finalEvalProof": [..]}."""


# ------------------------------------------------------------------ polynomial.MultiLin
def _fold_prefix(bk, n, r, p):
    mid = n // 2
    for i in range(mid):
        bk[i] = (bk[i] + r * (bk[i + mid] - bk[i])) % p
    return mid


def fold(m, r, p):
    """(*MultiLin).Fold on the list m, in place: the lower half is updated, the upper half stays; returns the new length."""
    return _fold_prefix(m, len(m), r, p)


def evaluate(m, coords, p):
    bk, n = list(m), len(m)
    for r in coords:
        n = _fold_prefix(bk, n, r, p)
    return bk[0] % p


def eq_loop(m, q, p):
    """(*MultiLin).Eq: the in-place doubling loop; m[0] holds the scale, len(m) = 2^len(q)."""
    n = len(q)
    assert len(m) == 1 << n
    for i in range(n):
        for j in range(1 << i):
            j0 = j << (n - i)
            j1 = j0 + (1 << (n - 1 - i))
            m[j1] = q[i] * m[j0] % p
            m[j0] = (m[j0] - m[j1]) % p
    return m


def eq_closed(q, scale, p):
    """v(h) = scale prod_i (bit_{n-1-i}(h) ? q[i] : 1 - q[i])."""
    n = len(q)
    out = []
    for h in range(1 << n):
        v = scale % p
        for i in range(n):
            v = v * (q[i] if (h >> (n - 1 - i)) & 1 else 1 - q[i]) % p
        out.append(v)
    return out


def eval_eq(q, h, p):
    res = 1
    for a, b in zip(q, h):
        res = res * (1 + 2 * a * b - a - b) % p
    return res % p


# ------------------------------------------------------------------ gates
class Gate:
    def __init__(self, f, degree):
        self.f, self.degree = f, degree

    def evaluate(self, p, ins):
        return self.f(*ins) % p


def _add(*x):
    return sum(x)


def _mul(*x):
    r = 1
    for v in x:
        r *= v
    return r


GATES = {
    "identity": Gate(lambda x: x, 1),
    "add": Gate(_add, 1),
    "sub": Gate(lambda x, y: x - y, 1),
    "neg": Gate(lambda x: -x, 1),
    "mul": Gate(_mul, 2),
    "mimc": Gate(lambda x, y: (x + y) ** 7, 7),             # mimcCipherGate with ark = 0 (gkr_test.go:563-584)
    "select-input-3": Gate(lambda *x: x[2], 1),            # _select(2)
}


# ------------------------------------------------------------------ circuit structure (gkr.go:691-778)
class Sorted:
    """topologicalSort: order[k] = circuit index of the k-th sorted wire; unique_outputs per circuit index."""

    def __init__(self, circuit):
        n = len(circuit)
        self.circuit = circuit
        outputs = [[] for _ in range(n)]
        self.unique_outputs = [0] * n
        for i, (_, ins) in enumerate(circuit):
            seen = set()
            for j in ins:
                outputs[j].append(i)
                if j not in seen:
                    seen.add(j)
                    self.unique_outputs[j] += 1
        status = [len(ins) for _, ins in circuit]
        least = 0
        while status[least] != 0:
            least += 1
        self.order = []
        for _ in range(n):
            self.order.append(least)
            status[least] = -1
            for o in outputs[least]:
                status[o] -= 1
                if status[o] == 0 and o < least:
                    least = o
            while least < n and status[least] != 0:
                least += 1

    def inputs(self, w):
        return self.circuit[w][1]

    def gate(self, w):
        return GATES["identity"] if not self.inputs(w) else (self.circuit[w][0] if isinstance(self.circuit[w][0], Gate) else GATES[self.circuit[w][0]])

    def is_input(self, w):
        return not self.inputs(w)

    def is_output(self, w):
        return self.unique_outputs[w] == 0

    def nb_claims(self, w):
        return 1 if self.is_output(w) else self.unique_outputs[w]

    def no_proof(self, w):
        return self.is_input(w) and self.nb_claims(w) == 1


def challenge_names(s, nvars, prefix=""):
    names = [prefix + "fC." + str(j) for j in range(nvars)]
    for i in range(len(s.order) - 1, -1, -1):
        w = s.order[i]
        if s.no_proof(w):
            continue
        wp = prefix + "w" + str(i) + "."
        if s.nb_claims(w) > 1:
            names.append(wp + "comb")
        names += [wp + "pSP." + str(k) for k in range(nvars)]
    return names


def complete(circuit, assignment, p):
    s = Sorted(circuit)
    a = list(assignment)
    n = len(next(v for v in a if v is not None))
    for w in s.order:
        if not s.is_input(w):
            a[w] = [s.gate(w).evaluate(p, [a[j][i] for j in s.inputs(w)]) for i in range(n)]
    return a


# ------------------------------------------------------------------ fiat-shamir/transcript.go
class Transcript:
    def __init__(self, hash_factory, names):
        self.hash_factory = hash_factory
        self.pos = {name: i for i, name in enumerate(names)}
        self.bindings = {name: [] for name in names}
        self.values = {}
        self.previous = None  # (position, value)

    def bind(self, name, value):
        if name not in self.pos:
            raise ValueError("challenge not recorded in the transcript")
        if name in self.values:
            raise ValueError("challenge already computed, cannot be binded to other values")
        self.bindings[name].append(bytes(value))

    def compute(self, name):
        if name not in self.pos:
            raise ValueError("challenge not recorded in the transcript")
        if name in self.values:
            return self.values[name]
        h = self.hash_factory()
        h.update(name.encode())
        if self.pos[name] != 0:
            if self.previous is None or self.previous[0] != self.pos[name] - 1:
                raise ValueError("the previous challenge is needed and has not been computed")
            h.update(self.previous[1])
        for b in self.bindings[name]:
            h.update(b)
        v = h.digest()
        self.values[name] = v
        self.previous = (self.pos[name], v)
        return v


class Field:
    def __init__(self, p, nbytes):
        self.p, self.nbytes = p, nbytes

    def to_bytes(self, v):
        return (v % self.p).to_bytes(self.nbytes, "big")

    def from_bytes(self, b):
        return int.from_bytes(b, "big") % self.p


def _next(F, t, bindings, names):
    name = names.pop(0)
    for v in bindings:
        t.bind(name, F.to_bytes(v))
    return F.from_bytes(t.compute(name))


# ------------------------------------------------------------------ one claim (eqTimesGateEvalSumcheckClaims)
class Claim:
    def __init__(self, p, gate, tables, points, degree=None):
        self.p, self.gate, self.points = p, gate, points
        self.degree = gate.degree if degree is None else degree
        self.inputs = [list(t) for t in tables]  # deep copies
        self.n = len(self.inputs[0])
        self.eq = None

    def vars_num(self):
        return len(self.points[0])

    def claims_num(self):
        return len(self.points)

    def combine(self, a):
        p, nvars = self.p, self.vars_num()
        self.eq = eq_loop([1] + [0] * ((1 << nvars) - 1), self.points[0], p)
        ai = a
        for k in range(1, self.claims_num()):
            new = eq_loop([ai % p] + [0] * ((1 << nvars) - 1), self.points[k], p)
            self.eq = [(x + y) % p for x, y in zip(self.eq, new)]
            if k + 1 < self.claims_num():
                ai = ai * a % p
        return self.compute_gj()

    def compute_gj(self):
        p, deg_gj = self.p, 1 + self.degree
        s = [self.eq] + self.inputs
        outer = self.n // 2
        gj = [0] * deg_gj
        for i in range(outer):
            ops = []
            for t in s:
                step = t[outer + i] - t[i]
                ops.append([(t[outer + i] + d * step) % p for d in range(deg_gj)])
            for d in range(deg_gj):
                gj[d] = (gj[d] + self.gate.evaluate(p, [o[d] for o in ops[1:]]) * ops[0][d]) % p
        return gj

    def next(self, r):
        for t in self.inputs + [self.eq]:
            _fold_prefix(t, self.n, r, self.p)
        self.n //= 2
        return self.compute_gj()

    def final_fold(self, r):
        """element 0 of every input table folded by r (length 2), in input order"""
        assert self.n == 2
        return [(t[0] + r * (t[1] - t[0])) % self.p for t in self.inputs]


def sumcheck_prove(F, claim, final_eval, t, prefix, base):
    nclaims, nvars = claim.claims_num(), claim.vars_num()
    names = ([prefix + "comb"] if nclaims >= 2 else []) + [prefix + "pSP." + str(i) for i in range(nvars)]
    for b in base:
        t.bind(names[0], b)
    comb = _next(F, t, [], names) if nclaims >= 2 else 0
    polys = [claim.combine(comb)]
    challenges = []
    for j in range(nvars - 1):
        challenges.append(_next(F, t, polys[j], names))
        polys.append(claim.next(challenges[j]))
    challenges.append(_next(F, t, polys[nvars - 1], names))
    return {"partialSumPolys": polys, "finalEvalProof": final_eval(challenges)}


def prove(F, circuit, assignment, hash_factory, prefix=""):
    p = F.p
    s = Sorted(circuit)
    nvars = (len(assignment[s.order[0]]) - 1).bit_length()
    t = Transcript(hash_factory, challenge_names(s, nvars, prefix))
    claims = {w: [] for w in range(len(circuit))}  # wire -> [(point, evaluation)]
    first = [F.from_bytes(t.compute(prefix + "fC." + str(j))) for j in range(nvars)]
    proof = [None] * len(circuit)
    base = []
    for i in range(len(circuit) - 1, -1, -1):
        w = s.order[i]
        if s.is_output(w):
            claims[w].append((first, evaluate(assignment[w], first, p)))
        if s.no_proof(w):
            proof[i] = {"partialSumPolys": [], "finalEvalProof": []}
        else:
            ins = s.inputs(w) or [w]
            claim = Claim(p, s.gate(w), [assignment[j] for j in ins], [pt for pt, _ in claims[w]])

            def final_eval(r, w=w, claim=claim):
                folded = claim.final_fold(r[-1])
                evals, no_more = [], {w}
                for k, j in enumerate(s.inputs(w)):
                    if j not in no_more:
                        no_more.add(j)
                        claims[j].append((r, folded[k]))
                        evals.append(folded[k])
                return evals

            proof[i] = sumcheck_prove(F, claim, final_eval, t, prefix + "w" + str(i) + ".", base)
            base = [F.to_bytes(v) for v in proof[i]["finalEvalProof"]]
        del claims[w]
    return proof


def _interpolate_eval(ys, r, p):
    """the polynomial through (k, ys[k]), k = 0 .. len(ys) - 1, at r"""
    res = 0
    for k, y in enumerate(ys):
        num, den = 1, 1
        for j in range(len(ys)):
            if j != k:
                num, den = num * (r - j) % p, den * (k - j) % p
        res = (res + y * num * pow(den, -1, p)) % p
    return res


def verify(F, circuit, assignment, proof, hash_factory, prefix=""):
    """Verify (gkr.go:635-689): assignment needs the input and output wires only. None, or the reference's error text."""
    p = F.p
    s = Sorted(circuit)
    nvars = (len(next(v for v in assignment if v is not None)) - 1).bit_length()
    t = Transcript(hash_factory, challenge_names(s, nvars, prefix))
    claims = {w: [] for w in range(len(circuit))}
    first = [F.from_bytes(t.compute(prefix + "fC." + str(j))) for j in range(nvars)]
    base = []
    for i in range(len(circuit) - 1, -1, -1):
        w = s.order[i]
        if s.is_output(w):
            claims[w].append((first, evaluate(assignment[w], first, p)))
        pw = proof[i]
        final = pw["finalEvalProof"]
        if s.no_proof(w):
            if final or pw["partialSumPolys"]:
                return "no proof allowed for input wire with a single claim"
            pt, ev = claims[w][0]
            if evaluate(assignment[w], pt, p) != ev % p:
                return "incorrect input wire claim"
        else:
            points, evals = [c[0] for c in claims[w]], [c[1] for c in claims[w]]
            wp = prefix + "w" + str(i) + "."
            names = ([wp + "comb"] if len(points) >= 2 else []) + [wp + "pSP." + str(k) for k in range(nvars)]
            for b in base:
                t.bind(names[0], b)
            comb = _next(F, t, [], names) if len(points) >= 2 else 0
            gjr = 0
            for e in reversed(evals):  # CombinedSum: the claimed evaluations as a polynomial in comb
                gjr = (gjr * comb + e) % p
            deg = 1 + s.gate(w).degree
            r = []
            for j in range(nvars):
                poly = pw["partialSumPolys"][j]
                if len(poly) != deg:
                    return "sumcheck proof rejected: malformed proof"
                gj = [(gjr - poly[0]) % p] + list(poly)
                r.append(_next(F, t, poly, names))
                gjr = _interpolate_eval(gj, r[j], p)
            ev = eval_eq(points[-1], r, p)
            for k in range(len(points) - 2, -1, -1):
                ev = (ev * comb + eval_eq(points[k], r, p)) % p
            if s.is_input(w):
                gate_ev = evaluate(assignment[w], r, p)
            else:
                ins, index, k = [], {}, 0
                for j in s.inputs(w):
                    if j not in index:
                        if k >= len(final):
                            return "sumcheck proof rejected: malformed final evaluation proof"
                        index[j] = k
                        claims[j].append((r, final[k]))
                        k += 1
                    ins.append(final[index[j]])
                if k != len(final):
                    return "sumcheck proof rejected: %d input wire evaluations given, %d expected" % (len(final), k)
                gate_ev = s.gate(w).evaluate(p, ins)
            if ev * gate_ev % p != gjr % p:
                return "sumcheck proof rejected: incompatible evaluations"
            base = [F.to_bytes(v) for v in final]
        del claims[w]
    return None
