"""The host plan of one run of the sorted pipeline (Pipeline::plan_run through gmsm_debug_run_layout, no device) against rows
recorded from the arithmetic the pipeline driver did inline before it was split into stages: tests/golden/pipeline_layout.json.
Every row is (group, num_cus, n, c, win_first, win_stride, glv, shared, flags, GMSM_OPT_REDUCE_SHAPE, GMSM_OPT_REDUCE_TAIL) and
either the 51 integers named by "fields" - window and entry counts, the accumulation and reduction geometry, the plane tail,
the sort layout, the bytes of every scratch buffer - or the text the run is refused with. The rows cover all six groups;
n from 2^10 to 2^27; the default window width and 8, 11, 16, 20; GLV half scalars; the shared bucket set of window tables; one
window and a strided piece of a window-sharded call; 256 and 64 compute units; forced two- and three-level reductions; the
three tail options against the three things a caller can take; and the refusals (GLV over registered bases, 2^31 entries,
the sort's 2^27-point and window-width limits, more than 256 windows)."""
import ctypes
import json
import os

import pytest

from conftest import ALL_GROUPS

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_layout.json")))
FIELDS = GOLDEN["fields"]
ROWS_OF = {gid: [r for r in GOLDEN["rows"] if r[0] == gid] for gid in range(len(ALL_GROUPS))}


def layout(gm, row):
    group, cus, n, c, wf, ws, glv, shared, flags, shape, tail, _ = row
    out = (ctypes.c_uint64 * len(FIELDS))()
    with gm.options(reduce_shape=shape, reduce_tail=tail):
        rc = gm._lib.load().gmsm_debug_run_layout(group, cus, n, c, wf, ws, glv, shared, flags, ctypes.addressof(out))
    return list(out) if rc == 0 else (rc, gm._lib.last_error())


def test_the_table_covers_what_it_says():
    assert len(FIELDS) == 51 and GOLDEN["columns"][-1] == "result"
    for gid in range(len(ALL_GROUPS)):
        rows = ROWS_OF[gid]
        assert len(rows) >= 35
        col = lambda i: {r[i] for r in rows}
        assert col(2) >= {1 << 10, 1 << 13, 1 << 14, 1 << 16, 1 << 20, 1 << 22, 1 << 24, (1 << 25) + 1, 1 << 27}
        assert col(3) >= {8, 11, 16, 20} and col(1) == {256, 64} and col(6) == {0, 1} and col(7) == {0, 1}
        assert (1, 4) in {(r[4], r[5]) for r in rows} and 1 in {r[-1][0] for r in rows if isinstance(r[-1], list)}
        assert len(col(9)) >= 3 and col(10) == {0, 1, 2}
        assert {r[8] >> 3 for r in rows} == {0, 1, 2} and {r[8] & 7 for r in rows} >= {0, 1, 2, 5}
    refusals = {r[-1] for r in GOLDEN["rows"] if isinstance(r[-1], str)}
    assert {t[:24] for t in refusals} == {"GLV plan over registered", "n must be < 2^31", "more than 2^27 points in",
                                          "window width too large f", "more than 256 windows in"}


@pytest.mark.parametrize("curve,which", ALL_GROUPS)
def test_layout_matches_the_recorded_rows(gm, curve, which):
    gid = gm._lib.GROUP_IDS[(curve, which)]
    for row in ROWS_OF[gid]:
        got, want = layout(gm, row), row[-1]
        if isinstance(want, str):
            assert got == (gm._lib.GMSM_ERR_ARG, want), row[:-1]
        else:
            assert got == want, (row[:-1], [(f, g, w) for f, g, w in zip(FIELDS, got, want) if g != w])

