"""fr/gkr (ecc/<curve>/fr/gkr/gkr.go), prover side, over libgmsm.so: Gate, Wire, Circuit, WireAssignment.Complete and Prove.
A Gate is an ordinary callable over + - * and unary -, traced once per input count into the straight-line program of
iop.Program; each wire's sumcheck claim is a device handle (gmsm_gkr_claim_new / _next / _final, include/gmsm.h) that keeps
the eq table and the copies of the gate's input assignments in HBM between the rounds, while the Fiat-Shamir transcript
runs on the host (fiatshamir.py, sumcheck.py). Proofs are the reference's, element for element. Verify is host arithmetic of
the size of a proof and is not part of this module."""
import ctypes
import functools
import operator

import numpy as np

from . import _lib
from . import fiatshamir
from . import iop
from . import sumcheck
from .curves import CURVES
from .polynomial import MultiLin, _check, _elems, _gid, _ptr, evaluate_device

GKR_MAX_INPUTS, GKR_MAX_DEGREE = 16, 15  # GMSM_GKR_MAX_INPUTS, GMSM_GKR_MAX_DEGREE


def _curve(curve):
    return CURVES[curve] if isinstance(curve, str) else curve


class Gate:
    """Gate(f, degree): f takes the gate's inputs only; degree is Gate.Degree(), an upper bound of f's total degree."""

    def __init__(self, f, degree):
        self.f, self.degree, self._codes = f, int(degree), {}

    def Degree(self):
        return self.degree

    def code(self, curve, m):
        key = (_curve(curve).name, m)
        if key not in self._codes:
            self._codes[key] = iop.trace(curve, lambda i, *x: self.f(*x), m)
        return self._codes[key]


def MulGate(n):
    return Gate(lambda *x: functools.reduce(operator.mul, x), n)


# gkr.go:849-934
Gates = {
    "identity": Gate(lambda x: x, 1),
    "add": Gate(lambda *x: functools.reduce(operator.add, x), 1),
    "sub": Gate(lambda x, y: x - y, 1),
    "neg": Gate(lambda x: -x, 1),
    "mul": MulGate(2),
}


class Wire:
    def __init__(self, Gate=None, Inputs=()):
        self.Gate, self.Inputs, self.nbUniqueOutputs = Gate, list(Inputs), 0

    def IsInput(self):
        return len(self.Inputs) == 0

    def IsOutput(self):
        return self.nbUniqueOutputs == 0

    def NbClaims(self):
        return 1 if self.IsOutput() else self.nbUniqueOutputs

    def noProof(self):
        return self.IsInput() and self.NbClaims() == 1


class Circuit(list):
    """a list of Wire"""


def topological_sort(c):
    """topologicalSort (gkr.go:691-778): the wires in order of dependence, as close to the given order as possible; sets
    nbUniqueOutputs and gives input wires the identity gate."""
    n = len(c)
    index = {id(w): i for i, w in enumerate(c)}
    outputs = [[] for _ in range(n)]
    for w in c:
        w.nbUniqueOutputs = 0
        if w.IsInput():
            w.Gate = Gates["identity"]
    for i, w in enumerate(c):
        seen = set()
        for inp in w.Inputs:
            j = index[id(inp)]
            outputs[j].append(i)
            if j not in seen:
                seen.add(j)
                inp.nbUniqueOutputs += 1
    status = [len(w.Inputs) for w in c]
    least = 0
    while status[least] != 0:
        least += 1
    order = []
    for _ in range(n):
        order.append(c[least])
        status[least] = -1
        for o in outputs[least]:
            status[o] -= 1
            if status[o] == 0 and o < least:
                least = o
        while least < n and status[least] != 0:
            least += 1
    return order


def ChallengeNames(sorted_wires, logNbInstances, prefix=""):
    names = [prefix + "fC." + str(j) for j in range(logNbInstances)]
    for i in range(len(sorted_wires) - 1, -1, -1):
        w = sorted_wires[i]
        if w.noProof():
            continue
        wp = prefix + "w" + str(i) + "."
        if w.NbClaims() > 1:
            names.append(wp + "comb")
        names += [wp + "pSP." + str(k) for k in range(logNbInstances)]
    return names


class WireAssignment:
    """The values of every wire across the 2^n instances: wire -> (2^n, fr_limbs) uint64 array (Montgomery limbs), or, with
    device=True, wire -> device pointer of such an array, produced on `stream`. Complete fills the wires that are not inputs
    through gmsm_iop_evaluate_expression, one call per wire; device arrays it makes are torch tensors kept by the assignment."""

    def __init__(self, curve, values, nb_instances=None, device=False, stream=0):
        self.curve, self.device, self.stream = _curve(curve), bool(device), stream
        self._values, self._owned = {}, {}
        for w, v in values.items():
            self[w] = v
        if device:
            if nb_instances is None:
                raise ValueError("a device assignment needs nb_instances")
            self.nb_instances = int(nb_instances)
        else:
            self.nb_instances = len(next(iter(self._values.values()))[1])

    def __setitem__(self, wire, value):
        self._values[id(wire)] = (wire, int(value) if self.device else _elems(self.curve, value))

    def __getitem__(self, wire):
        return self._values[id(wire)][1]

    def __contains__(self, wire):
        return id(wire) in self._values

    def NumInstances(self):
        return self.nb_instances

    def NumVars(self):
        return (self.nb_instances - 1).bit_length()

    def pointer(self, wire):
        v = self[wire]
        return v if self.device else v.ctypes.data

    def Complete(self, c):
        n, cv = self.nb_instances, self.curve
        for w in topological_sort(c):
            if w.IsInput():
                continue
            m = len(w.Inputs)
            if self.device:
                import torch
                t = torch.empty(n * cv.fr_limbs, dtype=torch.int64, device="cuda")
                self._owned[id(w)] = t
                iop.evaluate_expression_device(cv, w.Gate.code(cv, m), [self[i] for i in w.Inputs], n, [n] * m, [0] * m, [iop.Regular] * m,
                                               iop.Regular, t.data_ptr(), stream=self.stream)
                self[w] = t.data_ptr()
            else:
                out = np.zeros((n, cv.fr_limbs), dtype=np.uint64)
                iop._expression_call(cv, w.Gate.code(cv, m), None, [self[i].ctypes.data for i in w.Inputs], None, m, n, [n] * m, [0] * m,
                                     [iop.Regular] * m, iop.Regular, 0, _ptr(out), None)
                self[w] = out
        return self

    def to_host(self, wire):
        """the wire's values as a host array; of a device assignment, only the wires that Complete made"""
        if not self.device:
            return self[wire]
        import torch
        torch.cuda.synchronize()
        return self._owned[id(wire)].cpu().numpy().view(np.uint64).reshape(-1, self.curve.fr_limbs)

    def evaluate(self, wire, point):
        """assignment[wire].Evaluate(point): the value's limbs"""
        if self.device:
            return evaluate_device(self.curve, self[wire], self.nb_instances, point, self.stream)
        return MultiLin(self.curve, self[wire]).Evaluate(point)


class Claim:
    """eqTimesGateEvalSumcheckClaims (gkr.go:143-348) as a device handle: the sumcheck.Prove claims object of one wire.
    tables: the gate's input assignments (arrays, or device pointers with device=True), copied by the library."""

    def __init__(self, curve, gate, tables, nb_instances, points, device=False, stream=0, degree=None):
        self.curve, self.gate, self.tables, self.n = _curve(curve), gate, list(tables), int(nb_instances)
        self.points, self.device, self.stream = [_elems(self.curve, p) for p in points], bool(device), stream
        self.degree = gate.Degree() if degree is None else int(degree)
        self.handle = None

    def VarsNum(self):
        return self.points[0].shape[0]

    def ClaimsNum(self):
        return len(self.points)

    def Combine(self, combinationCoeff):
        c, m = self.curve, len(self.tables)
        code = self.gate.code(c, m)
        words = np.ascontiguousarray(code.words, dtype=np.uint32)
        consts = np.ascontiguousarray(code.consts, dtype=np.uint64).reshape(-1, c.fr_limbs)
        if not self.device:
            self.tables = [_elems(c, t) for t in self.tables]
        ptrs = (ctypes.c_void_p * m)(*[int(t) if self.device else t.ctypes.data for t in self.tables])
        pts = np.ascontiguousarray(np.concatenate(self.points) if self.points else np.zeros((0, c.fr_limbs)), dtype=np.uint64)
        comb = _elems(c, combinationCoeff, 1)
        gj = np.zeros((self.degree + 1, c.fr_limbs), dtype=np.uint64)
        handle = ctypes.c_uint64(0)
        _check(_lib.load().gmsm_gkr_claim_new(
            _gid(c), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(words), _ptr(consts) if len(consts) else None, len(consts),
            self.degree, None if self.device else ptrs, ptrs if self.device else None, m, self.n, _ptr(pts), len(self.points), _ptr(comb),
            self.stream or None, _ptr(gj), ctypes.byref(handle)))
        self.handle = handle.value
        return gj

    def Next(self, element):
        gj = np.zeros((self.degree + 1, self.curve.fr_limbs), dtype=np.uint64)
        _check(_lib.load().gmsm_gkr_claim_next(self.handle, _ptr(_elems(self.curve, element, 1)), _ptr(gj)))
        return gj

    def final(self, r):
        """element 0 of every input table folded by r, in input order"""
        out = np.zeros((len(self.tables), self.curve.fr_limbs), dtype=np.uint64)
        _check(_lib.load().gmsm_gkr_claim_final(self.handle, _ptr(_elems(self.curve, r, 1)), _ptr(out)))
        return out

    def ProveFinalEval(self, r):
        return self.final(r[-1])

    def release(self):
        if self.handle:
            h, self.handle = self.handle, None
            _check(_lib.load().gmsm_gkr_claim_release(h))


class _WireClaim(Claim):
    """a Claim that knows its wire: ProveFinalEval hands the evaluations of the distinct input wires on as new claims"""

    def __init__(self, manager, wire, **kw):
        a = manager.assignment
        ins = wire.Inputs or [wire]
        super().__init__(a.curve, wire.Gate, [a[w] for w in ins], a.nb_instances, [p for p, _ in manager.claims[id(wire)]],
                         device=a.device, stream=a.stream, **kw)
        self.manager, self.wire = manager, wire

    def ProveFinalEval(self, r):
        folded = self.final(r[-1])
        evaluations, no_more = [], {id(self.wire)}
        for k, w in enumerate(self.wire.Inputs):
            if id(w) not in no_more:  # the first occurrence of each distinct input wire, never the wire itself
                no_more.add(id(w))
                self.manager.add(w, r, folded[k])
                evaluations.append(folded[k])
        return evaluations


class _ClaimsManager:
    def __init__(self, c, assignment):
        self.assignment = assignment
        self.claims = {id(w): [] for w in c}  # wire -> [(evaluation point, claimed evaluation)]

    def add(self, wire, point, evaluation):
        self.claims[id(wire)].append((np.array(point, dtype=np.uint64).reshape(-1, self.assignment.curve.fr_limbs), evaluation))


def Prove(c, assignment, transcriptSettings, sorted_wires=None):
    """gkr.Prove (gkr.go:578-631): the proof, per sorted wire a sumcheck.Proof (empty for an input wire with one claim)."""
    cv = assignment.curve
    nb_vars = assignment.NumVars()
    if 1 << nb_vars != assignment.NumInstances():
        raise ValueError("number of instances must be power of 2")
    for w in c:
        if len(w.Inputs) > GKR_MAX_INPUTS:
            raise ValueError("a gate with %d inputs, more than %d" % (len(w.Inputs), GKR_MAX_INPUTS))
    order = sorted_wires if sorted_wires is not None else topological_sort(c)
    s = transcriptSettings
    if s.Transcript is None:
        names = ChallengeNames(order, nb_vars, s.Prefix)
        transcript, prefix = fiatshamir.NewTranscript(s.Hash, *names), ""  # setup() leaves transcriptPrefix empty here
        for b in s.BaseChallenges:
            transcript.Bind(names[0], b)
    else:
        transcript, prefix = s.Transcript, s.Prefix
    manager = _ClaimsManager(c, assignment)
    first = np.array([sumcheck.element_from_bytes(cv, transcript.ComputeChallenge(prefix + "fC." + str(j))) for j in range(nb_vars)],
                     dtype=np.uint64).reshape(-1, cv.fr_limbs)
    proof = [None] * len(c)
    base = []
    for i in range(len(c) - 1, -1, -1):
        wire = order[i]
        if wire.IsOutput():
            manager.add(wire, first, assignment.evaluate(wire, first))
        if wire.noProof():
            proof[i] = sumcheck.Proof([], [])
        else:
            claim = _WireClaim(manager, wire)
            try:
                proof[i] = sumcheck.Prove(claim, transcript, prefix + "w" + str(i) + ".", base)
            finally:
                claim.release()
            base = [sumcheck.element_bytes(cv, e) for e in proof[i].FinalEvalProof]
        del manager.claims[id(wire)]
    return proof
