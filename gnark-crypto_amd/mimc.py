"""fr/mimc (ecc/<curve>/fr/mimc/mimc.go) over libgmsm.so: the MiMC hash of the curve's scalar field in Miyaguchi-Preneel mode.

NewMiMC(curve) is the reference's hash.StateStorer with hashlib's method names beside Go's (update = Write, digest = Sum(nil)):
it sits over gmsm_mimc_hash, host arithmetic that never touches the device, and fits fiatshamir.Transcript as hash_factory
(`lambda: NewMiMC("bn254")`, or Factory("bn254")). SumBatch hashes many messages at once on the device (gmsm_mimc_sum_batch):
one lane per message. Elements cross the C ABI as Montgomery limbs; bytes are the reference's: canonical, big-endian on output,
big-endian on input unless byte_order="little"."""
import ctypes

import numpy as np

from . import _lib
from .polynomial import _check, _curve, _elems, _gid, _ptr, from_int, to_int

ErrInvalidEncoding = "invalid fr.Element encoding"
ErrInvalidLength = "invalid input length: must represent a list of field elements, expects a []byte of len m*BlockSize"
ErrInvalidState = "the provided newState does not represent a valid state"


def BlockSize(curve):
    return 8 * _curve(curve).fr_limbs


def GetConstants(curve):
    """mimc.GetConstants: the round constants as integers (110 for BN254, 111 for BLS12-381, 163 for BW6-761)."""
    c = _curve(curve)
    rounds = ctypes.c_uint(0)
    _check(_lib.load().gmsm_mimc_constants(_gid(c), None, ctypes.byref(rounds)))
    out = np.zeros((rounds.value, c.fr_limbs), dtype=np.uint64)
    _check(_lib.load().gmsm_mimc_constants(_gid(c), _ptr(out), None))
    return [to_int(c, row) for row in out]


def hash_elements(curve, elems, state=None):
    """gmsm_mimc_hash: the digest's limbs of the elements (Montgomery limbs, (len, fr_limbs)), continued from `state`."""
    c = _curve(curve)
    e = _elems(c, elems)
    out = np.zeros(c.fr_limbs, dtype=np.uint64)
    st = None if state is None else _elems(c, state, 1)
    _check(_lib.load().gmsm_mimc_hash(_gid(c), None if st is None else _ptr(st), _ptr(e) if len(e) else None, len(e), _ptr(out)))
    return out


class MiMC:
    def __init__(self, curve, byte_order="big"):
        if byte_order not in ("big", "little"):
            raise ValueError("byte_order is 'big' or 'little'")
        self.curve, self.byte_order = _curve(curve), byte_order
        self.block_size = self.digest_size = BlockSize(self.curve)
        self.Reset()

    def Reset(self):
        self.h, self.data = 0, []

    def Size(self):
        return self.block_size

    def BlockSize(self):
        return self.block_size

    def Write(self, p):
        """Blocks of BlockSize bytes, each a canonical element; input shorter than one block is left-padded with zeros.
        Nothing is taken in when the call fails."""
        p, bs = bytes(p), self.block_size
        if 0 < len(p) < bs:
            p = bytes(bs - len(p)) + p
        if len(p) % bs:
            raise ValueError(ErrInvalidLength)
        vals = [int.from_bytes(p[i:i + bs], self.byte_order) for i in range(0, len(p), bs)]
        if any(v >= self.curve.r for v in vals):
            raise ValueError(ErrInvalidEncoding)
        self.data += vals
        return len(p)

    update = Write

    def _checksum(self):
        c = self.curve
        if self.data:
            elems = np.array([from_int(c, v) for v in self.data], dtype=np.uint64)
            self.h = to_int(c, hash_elements(c, elems, from_int(c, self.h)))
        self.data = []  # Sum flushes the data already hashed
        return self.h

    def Sum(self, b=b""):
        return bytes(b) + self._checksum().to_bytes(self.block_size, "big")

    def digest(self):
        return self.Sum()

    def State(self):
        return self.Sum()

    def SetState(self, newState):
        newState = bytes(newState)
        if len(newState) != self.block_size:
            raise ValueError("the mimc state expects a state of %d bytes" % self.block_size)
        v = int.from_bytes(newState, "big")
        if v >= self.curve.r:
            raise ValueError(ErrInvalidState)
        self.h, self.data = v, []


def NewMiMC(curve, byte_order="big"):
    return MiMC(curve, byte_order)


def Factory(curve, byte_order="big"):
    """a hash_factory for fiatshamir.Transcript / fiatshamir.WithHash"""
    return lambda: MiMC(curve, byte_order)


def Sum(curve, msg):
    h = MiMC(curve)
    h.Write(msg)
    return h.Sum()


def SumBatch(curve, msgs, state=None):
    """The digests of count messages of len elements each, hashed on the device: msgs is (count, len, fr_limbs) Montgomery
    limbs on the host, the result (count, fr_limbs)."""
    c = _curve(curve)
    m = np.ascontiguousarray(msgs, dtype=np.uint64)
    if m.ndim != 3 or m.shape[2] != c.fr_limbs:
        raise ValueError("msgs must have shape (count, len, %d)" % c.fr_limbs)
    count, length = m.shape[:2]
    out = np.zeros((count, c.fr_limbs), dtype=np.uint64)
    st = None if state is None else _elems(c, state, 1)
    _check(_lib.load().gmsm_mimc_sum_batch(_gid(c), _ptr(m) if m.size else None, None, count, length, length, None if st is None else _ptr(st), None,
                                           _ptr(out), None))
    return out


def sum_batch_device(curve, d_msgs, count, length, stride, d_out, state=None, stream=0):
    """gmsm_mimc_sum_batch on device pointers: message i is the `length` elements at element offset i * stride of d_msgs."""
    c = _curve(curve)
    st = None if state is None else _elems(c, state, 1)
    _check(_lib.load().gmsm_mimc_sum_batch(_gid(c), None, d_msgs, int(count), int(length), int(stride), None if st is None else _ptr(st), stream or None,
                                           None, d_out))
