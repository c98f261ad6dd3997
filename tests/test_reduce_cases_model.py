"""Every case of tests/reduce_cases.py through the host model of the bucket reduction (tests/combine_model.py over Z_r), for
every launch shape tests/test_gpu_reduce_shapes.py runs on the device - (NB, log2L, levels) admissible, both combine
schedules: the model's total is sum (j + 1) b_j mod r, and the case produces the events it is named for at that shape. The
second check is what makes the device test sharp instead of lucky: a case that misses its events at some shape is a bug of
the generator."""
import pytest

import combine_model as cm
import reduce_cases as rc

CURVES = ["bn254", "bls12_381", "bw6_761"]
NW = 3  # populated bucket sets of the device test


def run(r, case, w, NB, log2L, three, we):
    grp = cm.Group(r, log=True)
    pad = NB - len(case.b[w])  # buckets only the top window reaches
    B = [v if v else None for v in case.b[w]] + [None] * pad
    stored = [bool(v) or i for v, i in zip(case.b[w], case.inf[w])] + [False] * pad
    total, info = cm.reduce_window(grp, B, stored, log2L, three, we)
    return total, info, set(grp.events), grp.events


def check_events(name, r, NBset, log2L, three, b, total, info, ev, events):
    L, N = 1 << log2L, cm.COMBINE_N
    NB = len(b)
    T = (NBset + L - 1) // L
    nblocks1 = (T + N - 1) // N
    has = lambda kernel, phase, kind: any(e[0] == kernel and e[1] == phase and e[3] == kind for e in ev)
    steps = lambda kernel, phase, kind: {e[2] for e in ev if e[0] == kernel and e[1] == phase and e[3] == kind}
    if name == "dense":
        assert not [e for e in ev if e[3] in ("P+P", "P-P")] and total is not None
    elif name == "all_equal":
        full = min(NB // L, N)  # full segments of the first combine block
        for phase in ("scan", "pairs"):  # k_combine_q's scan steps 0.., k_combine_we's pair sums 1..
            if any(e[1] == phase for e in ev if e[0] == "combine1"):
                want = {s for s in range(6) if (2 << s) <= full}
                got = steps("combine1", phase, "P+P")
                assert want <= ({s - 1 for s in got} if phase == "pairs" else got), (phase, want, got)
        nfull = NB // (N * L) if not three else 0  # full blocks that reach k_reduce2_q's scan
        assert {s for s in range(6) if (2 << s) <= nfull} <= steps("reduce2", "scan", "P+P")
        if three:
            assert {s for s in range(6) if (2 << s) <= min(NB // (N * L), N)} <= {
                s - (1 if has("combine2", "pairs", "P+P") else 0) for s in steps("combine2", "scan", "P+P") | steps("combine2", "pairs", "P+P")}
    elif name == "alternating":
        nseg = (NB + L - 1) // L  # segments with reachable buckets; the others are empty
        assert all(s is None for s in info["S"]) and all((w is not None) == (t < nseg) for t, w in enumerate(info["W"]))
        assert has("serial", "run", "P-P") and total is not None
    elif name == "zero_S":
        parks = [e for e in events if e[:2] == ("combine1", "park")]
        assert len(parks) == nblocks1 * (log2L + 6) and all(e[3] == "dbl_inf" for e in parks)
        if three:
            parks2 = [e for e in events if e[:2] == ("combine2", "park")]
            assert parks2 and all(e[3] == "dbl_inf" for e in parks2)
        assert not has("reduce2", "scan", "P+Q") and total is not None
    elif name == "zero_total":
        assert total is None and any(e[3] == "P-P" for e in ev)
    elif name.startswith("single@"):
        j = int(name.split("@")[1])
        assert [k for k, v in enumerate(b) if v] == [j] and total == (j + 1) * b[j] % r
    elif name in ("finish+", "finish-"):
        assert has("combine1", "finish", "P+P" if name[-1] == "+" else "P-P")
        assert (total is None) == (name[-1] == "-")  # nothing else is in the window
    elif name in ("finish2+", "finish2-"):
        kind = "P+P" if name[-1] == "+" else "P-P"
        if three:
            assert has("combine2", "finish", kind)
        else:
            assert has("reduce2", "finish", kind)
            assert name[-1] == "-" or has("reduce2", "tree", "P+P")
        assert (total is None) == (three and name[-1] == "-")  # P - P in the last step of the last combine ends the sum
    elif name == "stored_infinity":
        assert has("serial", "run", "P+inf") and total is not None
        assert has("serial", "run", "inf+inf") or NB == 2  # (a segment's last slot is the first the walk reads)
    else:
        assert name == "sparse"


@pytest.mark.parametrize("c", rc.C_VALUES)
@pytest.mark.parametrize("curve", CURVES)
def test_every_case_produces_its_events_at_every_shape(gm, curve, c):
    r = gm.CURVES[curve].r
    NB, NBset = 1 << (c - 1), rc.nbuckets(r.bit_length(), c)
    assert NBset == NB or (curve, c) == ("bn254", 2)
    seen = set()
    assert rc.shapes(NBset)
    for log2L, levels in rc.shapes(NBset):
        named = rc.cases(r, NB, log2L, levels, NW)
        seen |= {n.split("@")[0] for n in named}
        for name, case in named.items():
            for w in range(NW):
                want = rc.weighted(r, case.b[w]) or None
                for we in (False, True):
                    total, info, ev, events = run(r, case, w, NBset, log2L, levels == 3, we)
                    assert total == want, (name, w, log2L, levels, we)
                    check_events(name, r, NBset, log2L, levels == 3, case.b[w], total, info, ev, events)
    must = {"dense", "sparse", "all_equal", "alternating", "zero_S", "zero_total", "single", "stored_infinity"}
    if NB > 2:
        must |= {"finish+", "finish-"}
    if NB > 2 * 64 + 1:
        must |= {"finish2+", "finish2-"}
    assert must <= seen


def test_shapes_are_the_admissible_ones():
    """two levels: NB <= 64 * 64 L; three: NB > 64 L - and every c has a shape, 2^10 and 2^13 buckets have three-level ones"""
    assert [rc.nbuckets(254, c) for c in rc.C_VALUES] == [4, 64, 1024, 8192]  # BN254: c = 2 divides 254, the top window is full
    assert [rc.nbuckets(bits, c) for bits in (255, 377) for c in rc.C_VALUES] == [2, 64, 1024, 8192] * 2
    assert rc.shapes(4) == rc.shapes(2)
    got = {c: rc.shapes(1 << (c - 1)) for c in rc.C_VALUES}
    assert got[2] == got[7] == [(1, 2), (2, 2), (4, 2), (8, 2)]
    assert got[11] == [(1, 2), (2, 2), (4, 2), (8, 2), (1, 3), (2, 3)]
    assert got[14] == [(1, 2), (2, 2), (4, 2), (8, 2), (1, 3), (2, 3), (4, 3)]
