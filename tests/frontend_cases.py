"""Inputs for the tests of the stages between the digits and the buckets of the sorted MultiExp pipeline - the sort (k_decompose*,
k_part_hist / colscan / rowscan / scatter, k_fine_sort, k_heavy_hist / scan / place), the accumulation (k_accumulate_seg) and the
split-bucket fix-up (k_fixup_seg, k_fixup_seg_q, k_fixup_bucket, k_fixup_long): tests/test_frontend_cases_model.py shows on the
host that every case reaches the regime it is named for, tests/test_gpu_frontend_shapes.py runs them on the device.

The model. recode() is partitionScalars on Python ints (signed digits, no borrow out of the top window), recode_array() the same
on limb arrays; scalar_from_digits() / scalars_from_digit_matrix() go the other way and check the round trip. A scalar with the
digit d in window w puts its base (negated for d < 0) into bucket |d| - 1 of that window, so a list of bucket POPULATIONS fixes
the starts[] the sort must produce, and with the layout's `seg` which accumulation thread holds which part of which bucket
(thread t owns the entries [t seg, (t + 1) seg) of the window's sorted list; a bucket [lo, hi) is a chain over the threads
lo // seg .. (hi - 1) // seg). The order inside a bucket is the sort's own business and nothing here depends on it.

The cases (populations(); the predicate of each says what makes it that case):
    stage_exact   one coarse partition of exactly stage_cap references (all register slots of k_fine_sort<24>) and one of
                  stage_cap + 1 (the smallest the heavy kernels take); variants: the crowd spread over the partition's fine
                  buckets / all of it in one bucket
    heavy_rows    partitions of 4 HEAVY_SUB and 4 HEAVY_SUB + 1 references in one window (a last sub-run of one reference), a
                  heavy partition two windows further on and none between: heavy_prefix / heavy_item over windows without rows
    chains        a bucket of exactly seg references on a thread boundary (no partial); one that spills a single reference;
                  chains of 1, FIXUP_MAXWALK, FIXUP_MAXWALK + 1 followers; of 63, 64, 65, LONG_PIECE, LONG_PIECE + 1 and
                  2 LONG_PIECE + 1 links; the tail of one chain and the head of the next in one thread; chains that end on a
                  thread boundary; the 64- and the LONG_PIECE-link chain with seg references in every link; a ragged total
    gaps          occupied buckets 0, 1, 4, 5 and >= NB / 4 empty buckets apart, each with the boundary inside a thread's range
                  and on its edge; the last occupied bucket is NB - 1, after a long gap
Contents of `chains` (CONTENTS): distinct bases; one base through every chain bucket (equal links: every step of k_fixup_long's
tree is P + P); P and -P in equal numbers in every chain bucket (partial sums are small multiples of P, the bucket is a stored
infinity); every seventh base at infinity.

Expected values need no group arithmetic on the host: base i is [a_i]G, a_i = k0 + i k1 (the oracle's gen_points; 0 for a base
replaced by infinity, a_j for a copy of base j, r - a_j for its negative), so the total of window w is [sum_i a_i d_w(s_i)]G -
one oracle.scalar_mul per window."""
import ctypes
import json
import os
import random

import numpy as np

# the constants the cases are built round, with the line of gnark-crypto_amd/csrc/gmsm_kernels.h each comes from
PART_CHUNK = 12288    # constexpr uint32_t PART_CHUNK = 12288, PART_CHUNK_BIG = 16384;
HEAVY_SUB = 8192      # constexpr uint32_t HEAVY_SUB = 8192;
FIXUP_MAXWALK = 8     # constexpr uint32_t FIXUP_MAXWALK = 8;  // upper limit of the `maxwalk` argument of k_fixup_seg
LONG_PIECE = 256      # constexpr uint32_t LONG_PIECE = 256;   // links per item of the long-chain list
FINE_SLOTS = 24 * 1024  # k_fine_sort<24>, 1024 threads: the references a partition may have to stay in registers (stage_sort)

# where the device file runs the cases (tests/test_frontend_cases_model.py checks the same layouts on the host)
CASE_C = {"bn254": 13, "bw6_761": 16}   # chains and gaps: 2^12 / 2^15 buckets, no wider top window
CASE_SIZES = range(513, 1 << 17, 512)   # ... at the smallest of these n whose layout lets the case be built
SORT_C, SORT_SIZES = 13, [(1 << 17) - 3]  # stage_exact and heavy_rows: 16 partitions of 2^8 fine buckets


def case_windows(L):
    """the windows a case is run in: the first and a middle one"""
    return (0, L["nwd"] // 2)


FIELDS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_layout.json")))["fields"]
CONTENTS = ("distinct", "repeated", "plus_minus", "seventh_infinite")
MASK64 = (1 << 64) - 1


class CaseDoesNotFit(ValueError):
    """the case cannot be built for this layout (seg too large for the n, too few buckets ...)"""


# ------------------------------------------------------------------ the decomposition
def num_windows(fr_bits, c):
    return (fr_bits + c - 1) // c


def nbuckets(fr_bits, c):
    """buckets of one bucket set (Pipeline::make_plan; lastC of multiexp.go:690): 2^(max(c, lastC) - 1)"""
    nwin = num_windows(fr_bits, c)
    return 1 << (max(c, c + 1 - (nwin * c - fr_bits)) - 1)


def recode(curve, s, c):
    """signed digits of s, one per window, as partitionScalars takes them: a digit above 2^(c-1) - 1 borrows 2^c from the next
    window; the top window keeps what it is left with"""
    assert 2 <= c <= 24 and 0 <= s < curve.r
    nwin, mask, half = num_windows(curve.fr_bits, c), (1 << c) - 1, 1 << (c - 1)
    out, carry = [], 0
    for w in range(nwin):
        d = carry + ((s >> (c * w)) & mask)
        carry = 0
        if w + 1 < nwin and d >= half:
            d -= 1 << c
            carry = 1
        out.append(d)
    return out


def code(d):
    """the digit as the kernels store it: 0 / 2 d / 2 (-d - 1) + 1"""
    return 0 if d == 0 else 2 * d if d > 0 else 2 * (-d - 1) + 1


def scalar_from_digits(curve, digits, c):
    s = sum(d << (c * w) for w, d in enumerate(digits))
    assert 0 <= s < curve.r and recode(curve, s, c) == list(digits), (digits, c)
    return s


def limbs_from_ints(values, nlimbs):
    raw = b"".join(v.to_bytes(8 * nlimbs, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, nlimbs).copy()


def ints_from_limbs(limbs):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(limbs, dtype=np.uint64)]


def mont_limbs(curve, values):
    """scalars as the library takes them: Montgomery form, little-endian uint64 limbs"""
    R, r = curve.fr_R, curve.r
    return limbs_from_ints([v % r * R % r for v in values], curve.fr_limbs)


def ints_from_mont(curve, limbs):
    rinv = pow(curve.fr_R, -1, curve.r)
    return [v * rinv % curve.r for v in ints_from_limbs(limbs)]


def recode_array(curve, values, c):
    """recode() of many scalars at once: int64 digits[window][i]"""
    a = limbs_from_ints(values, curve.fr_limbs)
    nwin, mask, half = num_windows(curve.fr_bits, c), (1 << c) - 1, 1 << (c - 1)
    out = np.empty((nwin, a.shape[0]), dtype=np.int64)
    carry = np.zeros(a.shape[0], dtype=np.int64)
    for w in range(nwin):
        idx, sh = divmod(c * w, 64)
        v = a[:, idx] >> np.uint64(sh)
        if sh + c > 64 and idx + 1 < a.shape[1]:
            v = v | (a[:, idx + 1] << np.uint64(64 - sh))
        d = (v & np.uint64(mask)).astype(np.int64) + carry
        carry = np.zeros_like(carry)
        if w + 1 < nwin:
            carry = (d >= half).astype(np.int64)
            d = d - (carry << c)
        out[w] = d
    return out


def scalars_from_digit_matrix(curve, D, c):
    """scalar_from_digits() of every column of D[window][i]"""
    nwin, n = D.shape
    limbs = np.zeros((n, curve.fr_limbs + 1), dtype=np.uint64)
    borrow = np.zeros(n, dtype=np.int64)
    for w in range(nwin):  # signed digits -> the bits of the window: a negative one borrows 2^c from the next
        u = D[w] - borrow
        borrow = (u < 0).astype(np.int64)
        u = (u + (borrow << c)).astype(np.uint64)
        idx, sh = divmod(c * w, 64)
        limbs[:, idx] |= u << np.uint64(sh)
        if sh + c > 64:
            limbs[:, idx + 1] |= u >> np.uint64(64 - sh)
    assert not borrow.any(), "a negative scalar"
    vals = ints_from_limbs(limbs)
    assert all(0 <= v < curve.r for v in vals)
    assert (recode_array(curve, vals, c) == D).all()
    return vals


def bucket_populations(D, NB):
    """populations[window][bucket] of a digit matrix: the digit d goes to bucket |d| - 1"""
    out = np.zeros((D.shape[0], NB), dtype=np.int64)
    for w in range(D.shape[0]):
        b = np.abs(D[w][D[w] != 0]) - 1
        assert b.size == 0 or b.max() < NB
        out[w] = np.bincount(b, minlength=NB)
    return out


# ------------------------------------------------------------------ the layout
def layout(gm, gid, num_cus, n, c, shared=0, resident=0):
    """gmsm_debug_run_layout (host arithmetic only) for all windows of an n-point run, by the field names of
    tests/golden/pipeline_layout.json; with the point count, the width and the bucket count"""
    out = (ctypes.c_uint64 * len(FIELDS))()
    rc = gm._lib.load().gmsm_debug_run_layout(gid, num_cus, n, c, 0, 1, 0, shared, resident, ctypes.addressof(out))
    if rc:
        raise RuntimeError(gm._lib.last_error())
    L = dict(zip(FIELDS, (int(v) for v in out)))
    L.update(n_points=n, c=c, NB=1 << L["log2NB"], num_cus=num_cus)
    return L


def spans(pops, seg):
    """(bucket, lo, hi, first thread, last thread) of every occupied bucket"""
    out, lo = [], 0
    for b, p in enumerate(pops):
        if p:
            out.append((b, lo, lo + p, lo // seg, (lo + p - 1) // seg))
            lo += p
    return out


def partition_populations(pops, fbits):
    return np.asarray(pops, dtype=np.int64).reshape(-1, 1 << fbits).sum(axis=1)


# ------------------------------------------------------------------ prescribed populations
class _Laying:
    """populations laid down in bucket order, with the entry position reached"""

    def __init__(self, NB, seg):
        self.pop, self.b, self.pos, self.seg = [0] * NB, 0, 0, seg

    def put(self, size):
        if self.b >= len(self.pop):
            raise CaseDoesNotFit("out of buckets")
        assert size > 0
        self.pop[self.b] = size
        self.b += 1
        self.pos += size

    def skip(self, empty):
        self.b += empty

    def to_offset(self, off):
        """a filler bucket that brings the position to `off` inside a thread's range (none if it is there)"""
        fill = (off - self.pos) % self.seg
        if fill:
            self.put(fill)

    def chain(self, links, ends_on_edge=False):
        """a bucket over exactly `links` threads from the current position; it ends 3 entries into its last thread or on its edge"""
        first = self.seg - self.pos % self.seg
        self.put(first + (links - 2) * self.seg + (self.seg if ends_on_edge else 3))


CHAIN_LINKS = (2, FIXUP_MAXWALK + 1, FIXUP_MAXWALK + 2, 63, 64, 65, LONG_PIECE, LONG_PIECE + 1, 2 * LONG_PIECE + 1)
GAPS = (0, 1, 4, 5)


def populations(L, name, variant=None):
    """{window offset: populations of every bucket, in bucket order} of a named case for a layout; offset 0 is the case window"""
    seg, NB, fbits, cap = L["seg"], L["NB"], L["fbits"], L["stage_cap"]
    if NB != 1 << (L["c"] - 1):
        raise CaseDoesNotFit("the bucket set is wider than the lower windows reach")
    if seg < 8:
        raise CaseDoesNotFit("seg < 8")
    nf = 1 << fbits
    if name == "chains":
        q = _Laying(NB, seg)
        q.put(seg)                        # a whole thread's range: stored by the accumulation, no partial
        q.put(seg + 1)                    # spills one reference: 1 follower; the next chain's head shares the follower's thread
        q.chain(FIXUP_MAXWALK + 1)        # FIXUP_MAXWALK followers: walked by the head
        q.put(2)                          # a whole bucket between a tail and a head in one thread
        q.chain(FIXUP_MAXWALK + 2)        # one more: handed to the list
        q.chain(63)
        q.to_offset(0)
        q.chain(64, ends_on_edge=True)    # seg references in every link
        q.chain(65)
        q.to_offset(0)
        q.chain(LONG_PIECE, ends_on_edge=True)
        q.chain(LONG_PIECE + 1)           # a second piece of one link
        q.chain(2 * LONG_PIECE + 1)
        q.put(1)
        if q.pos % seg == 0:
            q.put(1)
        return {0: q.pop}
    if name == "gaps":
        q = _Laying(NB, seg)
        for on_edge in (False, True):
            for gap in GAPS + (NB // 4,):
                q.to_offset(0)
                q.put(seg if on_edge else 3)  # the boundary to the next occupied bucket: on the thread's edge / inside its range
                q.skip(gap)
                if gap == NB // 4 and on_edge:
                    if q.b > NB - 1:
                        raise CaseDoesNotFit("out of buckets")
                    q.b = NB - 1
                q.put(seg + 2)
        if q.b != NB:
            raise CaseDoesNotFit("the last bucket is not NB - 1")
        return {0: q.pop}
    if name == "stage_exact":
        if L["nparts"] < 5 or fbits < 1 or cap != FINE_SLOTS:
            raise CaseDoesNotFit("needs nparts >= 5, fbits >= 1 and the staging slots of k_fine_sort<24>")
        pop = np.zeros((L["nparts"], nf), dtype=np.int64)
        pop[:, 0] = 3  # every other partition: a few references
        for p, total in ((1, cap), (3, cap + 1)):
            if variant == "spread":
                pop[p] = total // nf
                pop[p, : total % nf] += 1
            else:
                pop[p] = 0
                pop[p, nf // 2 if p == 1 else nf - 1] = total
        return {0: [int(v) for v in pop.reshape(-1)]}
    if name == "heavy_rows":
        if L["nparts"] < 5 or fbits < 1 or 3 * HEAVY_SUB + 5 <= cap:
            raise CaseDoesNotFit("needs nparts >= 5, fbits >= 1 and stage_cap < 3 HEAVY_SUB + 5")
        pop = np.zeros((L["nparts"], nf), dtype=np.int64)
        pop[:, 1 % nf] = 2
        pop[1] = 4 * HEAVY_SUB // nf                      # spread
        pop[1, : 4 * HEAVY_SUB % nf] += 1
        pop[L["nparts"] - 1] = (2 * HEAVY_SUB) // nf     # half spread, half in the last bucket
        pop[L["nparts"] - 1, : (2 * HEAVY_SUB) % nf] += 1
        pop[L["nparts"] - 1, nf - 1] += 2 * HEAVY_SUB + 1
        second = np.zeros((L["nparts"], nf), dtype=np.int64)
        second[:, 0] = 1
        second[2] = (3 * HEAVY_SUB + 5) // nf
        second[2, : (3 * HEAVY_SUB + 5) % nf] += 1
        return {0: [int(v) for v in pop.reshape(-1)], 2: [int(v) for v in second.reshape(-1)]}
    raise KeyError(name)


def fit(gm, gid, num_cus, name, c, sizes, variant=None, shared=0):
    """(layout, populations) at the smallest n of `sizes` whose layout lets the case be built; CaseDoesNotFit if none does.
    shared: the one bucket set of window tables, filled by the digits of all windows below the top"""
    why = None
    for n in sizes:
        L = layout(gm, gid, num_cus, n, c, shared=shared, resident=shared)
        try:
            pops = populations(L, name, variant)
            room = n * (L["nwd"] - 1) if shared else n
            need = max(sum(p) for p in pops.values())
            if need > room:
                raise CaseDoesNotFit(f"{need} references, room for {room} (seg {L['seg']})")
            if shared and L["entries"] // L["NB"] < 2 * L["seg"]:
                raise CaseDoesNotFit("the shared set is not crowded enough for k_fixup_bucket")
            return L, pops
        except CaseDoesNotFit as e:
            why = e
    raise CaseDoesNotFit(f"{name} at c = {c}, {num_cus} CUs: {why}")


# ------------------------------------------------------------------ what makes a case that case
def check_chains(L, pops):
    seg = L["seg"]
    sp = spans(pops, seg)
    chains = [s for s in sp if s[4] > s[3]]
    links = {t1 - t0 + 1 for _, _, _, t0, t1 in chains}
    assert set(CHAIN_LINKS) <= links, sorted(links)
    assert any(hi - lo == seg and lo % seg == 0 for _, lo, hi, _, _ in sp), "no bucket of exactly seg on a boundary"
    assert any(hi - lo == seg + 1 and lo % seg == 0 for _, lo, hi, _, _ in sp), "no bucket that spills one reference"
    assert {s[4] for s in chains} & {s[3] for s in chains}, "no thread with the tail of one chain and the head of the next"
    assert any(hi % seg == 0 for _, _, hi, _, _ in chains), "no chain ends on a thread boundary"
    for m in (64, LONG_PIECE):
        assert any(lo % seg == 0 and hi - lo == m * seg for _, lo, hi, _, _ in chains), f"no chain of {m} equal links"
    total = sum(pops)
    assert total % seg != 0 and (total + seg - 1) // seg <= L["tpw"]


def check_shared_chains(L, pops):
    check_chains(L, pops)
    assert L["nw"] == 1 and L["entries"] == L["nwd"] * L["n_points"]
    assert L["entries"] // L["NB"] >= 2 * L["seg"], "k_fixup_seg, not k_fixup_bucket"  # stage_fixup


def check_gaps(L, pops):
    seg, NB = L["seg"], L["NB"]
    sp = spans(pops, seg)
    seen = set()
    for (b0, _, hi, _, _), (b1, lo, _, _, _) in zip(sp, sp[1:]):
        assert hi == lo
        gap = b1 - b0 - 1
        seen.add((gap if gap < NB // 4 else "long", lo % seg == 0))
    for g in GAPS + ("long",):  # k_accumulate_seg steps over up to 4 empty buckets and bisects from 5 on
        assert (g, False) in seen and (g, True) in seen, (g, sorted(seen, key=str))
    assert sp[-1][0] == NB - 1 and sp[-1][0] - sp[-2][0] - 1 >= NB // 4
    assert sum(pops) <= L["entries"]


def check_stage_exact(L, pops, variant):
    cap, nf = L["stage_cap"], 1 << L["fbits"]
    assert cap == FINE_SLOTS and L["nparts"] >= 5 and L["fbits"] >= 1 and L["entries"] > cap  # (n > stage_cap: the heavy kernels are launched)
    pp = partition_populations(pops, L["fbits"])
    per = np.asarray(pops).reshape(-1, nf)
    for total in (cap, cap + 1):
        hit = np.nonzero(pp == total)[0]
        assert hit.size == 1, (total, pp)
        occupied = int((per[hit[0]] > 0).sum())
        assert occupied == (nf if variant == "spread" else 1), (variant, occupied)
    assert (pp > cap).sum() == 1


def check_heavy_rows(L, allpops, w):
    cap, fbits = L["stage_cap"], L["fbits"]
    pp = [partition_populations(p, fbits) for p in allpops]
    for total, subruns, last in ((4 * HEAVY_SUB, 4, HEAVY_SUB), (4 * HEAVY_SUB + 1, 5, 1)):
        assert total > cap and (pp[w] == total).sum() == 1
        assert -(-total // HEAVY_SUB) == subruns and total - (subruns - 1) * HEAVY_SUB == last
    assert (pp[w] > cap).sum() == 2 and (pp[w + 2] > cap).sum() == 1 and (pp[w + 1] > cap).sum() == 0
    assert all((pp[k] > cap).sum() == 0 for k in range(len(pp)) if k not in (w, w + 2))
    assert L["entries"] > cap


# ------------------------------------------------------------------ the unforced shapes of the sort
def _log2ceil(n):
    return (n - 1).bit_length()


def _unclamped_fbits(L):
    return max(0, min(L["part_log2"] + L["log2NB"] - _log2ceil(L["entries"]), L["log2NB"], 15))


UNFORCED = {  # (n, c): (what it selects, the condition on the layout)
    (12287, 13): ("one chunk, one code short of full", lambda L: L["d16"] and L["pchunks"] == 1 and L["entries"] == L["pchunk_len"] - 1),
    (12288, 13): ("one full chunk: the vector path", lambda L: L["d16"] and L["pchunks"] == 1 and L["entries"] == L["pchunk_len"] and L["entries"] % 8 == 0),
    (12289, 13): ("a second chunk of one code", lambda L: L["d16"] and L["pchunks"] == 2 and L["entries"] == L["pchunk_len"] + 1),
    (3 * 12288 + 5, 13): ("16-bit codes, full chunks, every window after the first misaligned",
                          lambda L: L["d16"] and L["pchunks"] == 4 and L["entries"] % 8 != 0 and L["entries"] % 2 == 1),
    (65541, 17): ("32-bit codes, n mod 4 != 0", lambda L: not L["d16"] and L["pchunks"] > 2 and L["entries"] % 4 != 0),
    **{(n, c): ("fbits = 0: one bucket per partition", lambda L: L["fbits"] == 0 and L["nparts"] == L["NB"])
       for n in (1 << 16, (1 << 16) + 3) for c in (2, 3, 4)},
    **{(n, 20): ("fbits + lidx clamped to 32", lambda L: L["fbits"] + L["lidx"] == 32 and _unclamped_fbits(L) + L["lidx"] > 32 and not L["d16"])
       for n in ((1 << 16) + 1, 1 << 17, (1 << 17) + 1)},
}


def check_unforced(L):
    what, holds = UNFORCED[(L["n_points"], L["c"])]
    assert L["pchunk_len"] == PART_CHUNK and L["entries"] == L["n_points"] and holds(L), (what, L)


# ------------------------------------------------------------------ inputs and expected values
_POINTS = {}


class Bases:
    """base i = [k0 + i k1]G, except `changed`: i -> ("inf",) | ("copy", j) | ("neg", j) with base j unchanged"""

    def __init__(self, curve, n, k0, k1, changed=None):
        self.curve, self.n, self.k0, self.k1, self.changed = curve, n, k0 % curve.r, k1 % curve.r, dict(changed or {})
        assert all(len(v) == 1 or v[1] not in self.changed for v in self.changed.values())

    def multiplier(self, i):
        r = self.curve.r
        how = self.changed.get(i)
        if how is None:
            return (self.k0 + i * self.k1) % r
        return 0 if how[0] == "inf" else self.multiplier(how[1]) if how[0] == "copy" else (r - self.multiplier(how[1])) % r

    def points(self, o, nthreads=8):
        key = (o.name, self.k0, self.k1)  # base i does not depend on n: the longest array made so far serves the shorter ones
        if key not in _POINTS or len(_POINTS[key]) < self.n:
            _POINTS[key] = o.gen_points(self.n, self.k0, self.k1, nthreads=nthreads)
        pts = _POINTS[key][: self.n].copy()
        fl, cl, p = self.curve.fp_limbs, o.coord_limbs, self.curve.p
        for i, how in self.changed.items():
            if how[0] == "inf":
                pts[i] = 0
            else:
                pts[i] = pts[how[1]]
                if how[0] == "neg":
                    for lo in range(cl, 2 * cl, fl):
                        y = (p - int.from_bytes(pts[i, lo:lo + fl].tobytes(), "little")) % p
                        pts[i, lo:lo + fl] = [(y >> (64 * k)) & MASK64 for k in range(fl)]
        return pts

    def weighted(self, d):
        """sum_i a_i d_i mod r for int64 weights d"""
        d = np.asarray(d, dtype=np.int64)
        assert d.shape == (self.n,) and self.n < 1 << 20 and np.abs(d).max(initial=0) < 1 << 24
        total = self.k0 * int(d.sum()) + self.k1 * int((d * np.arange(self.n, dtype=np.int64)).sum())
        for i in self.changed:
            total += (self.multiplier(i) - (self.k0 + i * self.k1)) * int(d[i])
        return total % self.curve.r

    def weighted_ints(self, values):
        """sum_i a_i v_i mod r for Python ints"""
        return sum(self.multiplier(i) * v for i, v in enumerate(values)) % self.curve.r


def expected_affine(o, k):
    """affine Montgomery limbs of [k]G, None for the point at infinity"""
    return None if k == 0 else o.jac_to_affine(o.scalar_mul(o.generator, int(k)))


def check_totals(o, totals, want, tag):
    """XYZZ window totals of the device against expected_affine() values, limb for limb"""
    cl = o.coord_limbs
    assert len(totals) == len(want), tag
    for w, (row, exp) in enumerate(zip(totals, want)):
        zz = row[2 * cl:3 * cl]
        if exp is None:
            assert not zz.any(), (tag, w, "expected infinity")
        else:
            assert zz.any(), (tag, w, "infinity")
            assert (o.jac_to_affine(o.xyzz_to_jac(row)) == exp).all(), (tag, w)


def _seed(*tag):
    return random.Random("/".join(str(t) for t in tag)).getrandbits(64)


def uniform_scalars(curve, n, *tag):
    rng = random.Random(_seed("uniform", curve.name, n, *tag))
    return [rng.randrange(curve.r) for _ in range(n)]


def case_digits(curve, L, pops, w, *tag):
    """digits[window][i] of n scalars: the windows w + offset hold the prescribed populations (the references of a bucket scattered
    over the indices, both signs where the bucket has both; scalars left over have the digit 0 there), the other windows below the
    top seeded uniform non-zero digits (positive in the last of them: the scalar is not negative), the top window 0"""
    n, c, NB = L["n_points"], L["c"], L["NB"]
    nwin, half = L["nwd"], 1 << (c - 1)
    assert nwin == num_windows(curve.fr_bits, c) and nwin >= 6 and all(0 <= w + off < nwin - 2 for off in pops)
    rng = np.random.default_rng(_seed("digits", curve.name, n, c, w, *tag))
    D = rng.integers(-half, half - 1, size=(nwin, n), dtype=np.int64)
    D += D >= 0  # -half .. -1, 1 .. half - 1
    D[nwin - 2] = np.abs(D[nwin - 2])
    D[nwin - 2][D[nwin - 2] == half] = 1
    D[nwin - 1] = 0
    for off, pop in pops.items():
        pop = np.asarray(pop, dtype=np.int64)
        assert pop.shape == (NB,) and pop.sum() <= n
        mag = np.zeros(n, dtype=np.int64)
        mag[: pop.sum()] = np.repeat(np.arange(1, NB + 1, dtype=np.int64), pop)
        mag = mag[rng.permutation(n)]
        sign = np.where(rng.integers(0, 2, size=n) == 1, -1, 1)
        sign[mag == half] = -1  # bucket NB - 1 is reached by the digit -2^(c-1) only
        D[w + off] = mag * sign
    got = bucket_populations(D, NB)
    assert all((got[w + off] == np.asarray(pop)).all() for off, pop in pops.items())
    return D


def chain_contents(curve, L, pops, d, content, k0, k1):
    """Bases for a `chains` window with the digits d: see CONTENTS; `repeated` and `plus_minus` also make the digits of a chain
    bucket positive, so that all its references add the same point (or the point and its negative in equal numbers)"""
    n, seg = L["n_points"], L["seg"]
    d = d.copy()
    changed = {}
    if content == "seventh_infinite":
        changed = {i: ("inf",) for i in range(0, n, 7)}
    elif content in ("repeated", "plus_minus"):
        rng = random.Random(_seed("contents", curve.name, n, content))
        for b, lo, hi, t0, t1 in spans(pops, seg):
            if t1 == t0:
                continue
            idx = [int(i) for i in np.nonzero(np.abs(d) == b + 1)[0]]
            assert len(idx) == hi - lo and b + 1 < 1 << (L["c"] - 1)
            d[idx] = b + 1
            rng.shuffle(idx)
            rest = idx[1:]
            for pos, i in enumerate(rest):  # plus_minus: the bucket's own base and half of the others (rounded down) stay P
                changed[i] = ("neg" if content == "plus_minus" and pos < (len(idx) // 2) else "copy", idx[0])
    else:
        assert content == "distinct"
    return Bases(curve, n, k0, k1, changed), d


def shared_digits(curve, L, pop, *tag):
    """digits[window][i] whose values over ALL windows have the populations `pop` (the shared bucket set of window tables): positive
    digits scattered over the windows below the top, 0 elsewhere"""
    n, c, NB, nwin = L["n_points"], L["c"], L["NB"], L["nwd"]
    pop = np.asarray(pop, dtype=np.int64)
    slots = n * (nwin - 1)
    assert pop.shape == (NB,) and pop.sum() <= slots and not pop[(1 << (c - 1)) - 1:].any()
    rng = np.random.default_rng(_seed("shared", curve.name, n, c, *tag))
    flat = np.zeros(slots, dtype=np.int64)
    flat[: pop.sum()] = np.repeat(np.arange(1, NB + 1, dtype=np.int64), pop)
    D = np.zeros((nwin, n), dtype=np.int64)
    D[: nwin - 1] = flat[rng.permutation(slots)].reshape(nwin - 1, n)
    assert (bucket_populations(D, NB).sum(axis=0) == pop).all()
    return D
