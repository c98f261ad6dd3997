"""fr/sumcheck.Prove (ecc/<curve>/fr/sumcheck/sumcheck.go:44-123), generic over a claims object with Combine(a), Next(r),
ProveFinalEval(r), VarsNum(), ClaimsNum() - on the device that is gkr's claim handle; the Fiat-Shamir steps between the
rounds run here, on the host, with the reference's challenge names and binding order. Elements are Montgomery limb arrays."""
from collections import namedtuple

import numpy as np

from . import fiatshamir
from .polynomial import from_int, to_int

Proof = namedtuple("Proof", ["PartialSumPolys", "FinalEvalProof"])


def element_bytes(c, limbs):
    """fr.Element.Bytes(): the value, big-endian, fr.Bytes long"""
    return to_int(c, limbs).to_bytes(c.fr_limbs * 8, "big")


def element_from_bytes(c, b):
    """fr.Element.SetBytes: big-endian, reduced"""
    return from_int(c, int.from_bytes(b, "big"))


def _next(c, transcript, bindings, remaining):
    name = remaining.pop(0)
    for b in bindings:
        transcript.Bind(name, element_bytes(c, b))
    return element_from_bytes(c, transcript.ComputeChallenge(name))


def Prove(claims, transcript, prefix="", base_challenges=()):
    """transcript: a fiatshamir.Transcript that knows the names prefix + "comb" (two claims or more) and prefix + "pSP.i", or a
    hash factory, from which one is made (settings.Transcript == nil). claims.curve names the field."""
    c = claims.curve
    nclaims, nvars = claims.ClaimsNum(), claims.VarsNum()
    names = ([prefix + "comb"] if nclaims >= 2 else []) + [prefix + "pSP." + str(i) for i in range(nvars)]
    if not isinstance(transcript, fiatshamir.Transcript):
        transcript = fiatshamir.NewTranscript(transcript, *names)
    for b in base_challenges:
        transcript.Bind(names[0], b)
    comb = _next(c, transcript, [], names) if nclaims >= 2 else np.zeros(c.fr_limbs, dtype=np.uint64)
    polys = [claims.Combine(comb)]
    challenges = []
    for j in range(nvars - 1):
        challenges.append(_next(c, transcript, polys[j], names))
        polys.append(claims.Next(challenges[j]))
    challenges.append(_next(c, transcript, polys[nvars - 1], names))
    return Proof(polys, claims.ProveFinalEval(challenges))
