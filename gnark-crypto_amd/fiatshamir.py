"""fiat-shamir/transcript.go:20-127 on the host: a challenge is H(name || previous challenge || bound values), the previous
one left out for the first name. hash_factory() returns a fresh object with update / digest, such as hashlib.sha256 (the
reference resets one hash.Hash instead). The three errors are ValueErrors with the reference's texts."""

ErrChallengeNotFound = "challenge not recorded in the transcript"
ErrChallengeAlreadyComputed = "challenge already computed, cannot be binded to other values"
ErrPreviousChallengeNotComputed = "the previous challenge is needed and has not been computed"


class Transcript:
    def __init__(self, hash_factory, *names):
        self.hash_factory = hash_factory
        self.challenges = {name: {"position": i, "bindings": [], "value": None} for i, name in enumerate(names)}
        self.previous = None

    def Bind(self, challengeID, bValue):
        ch = self.challenges.get(challengeID)
        if ch is None:
            raise ValueError(ErrChallengeNotFound)
        if ch["value"] is not None:
            raise ValueError(ErrChallengeAlreadyComputed)
        ch["bindings"].append(bytes(bValue))

    def ComputeChallenge(self, challengeID):
        ch = self.challenges.get(challengeID)
        if ch is None:
            raise ValueError(ErrChallengeNotFound)
        if ch["value"] is not None:
            return ch["value"]
        h = self.hash_factory()
        h.update(challengeID.encode())
        if ch["position"] != 0:
            if self.previous is None or self.previous["position"] != ch["position"] - 1:
                raise ValueError(ErrPreviousChallengeNotComputed)
            h.update(self.previous["value"])
        for b in ch["bindings"]:
            h.update(b)
        ch["value"] = bytes(h.digest())
        self.previous = ch
        return ch["value"]


def NewTranscript(hash_factory, *names):
    return Transcript(hash_factory, *names)


class Settings:
    """fiatshamir.Settings (settings.go): a transcript to continue under a prefix, or a hash to start one from."""

    def __init__(self, Hash=None, Transcript=None, Prefix="", BaseChallenges=()):
        self.Hash, self.Transcript, self.Prefix, self.BaseChallenges = Hash, Transcript, Prefix, list(BaseChallenges)


def WithHash(hash_factory, *baseChallenges):
    return Settings(Hash=hash_factory, BaseChallenges=baseChallenges)


def WithTranscript(transcript, prefix, *baseChallenges):
    return Settings(Transcript=transcript, Prefix=prefix, BaseChallenges=baseChallenges)
