"""The host arithmetic of gmsm_fflonk.h without a GPU and outside python: tests/c/fflonk_host_check.hip, a stand-alone
program built with AddressSanitizer on its host side, prints FflonkField's divisors, root of one, extended sets, both
sets of claimed values (from chain remainders it computes by plain synthetic division), true length of w, index tables
and refusal codes on the three scalar fields, then the plan, tables, claimed values and refusal codes of the same pipeline in
shplonk's singleton form; they must equal tests/fflonk_model.py and tests/shplonk_model.py, and the sanitizer must stay
silent."""
import os
import subprocess

import pytest

import fflonk_model as fm
import shplonk_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
PACKS, POINTS = [[[1, 2, 3], [4, 5]], [[7], [], [1, 1], [2, 0, 9, 4], [6]]], [[3, 5], [2]]  # as in the program
S_POLYS, S_POINTS = [[1, 2, 3], [4, 5], [7]], [[3, 5], [2], [2, 9]]  # its singleton form: more points than coefficients in the third


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc is missing: the check cannot be built")
    exe = str(tmp_path_factory.mktemp("fflonk_host") / "fflonk_host_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "gnark-crypto_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "fflonk_host_check.hip")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    out = {}
    for blk in run.stdout.split("field ")[1:]:
        lines = blk.strip().split("\n")
        out[lines[0]] = [l.split() for l in lines[1:]]
    return out


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bw6_761"])
def test_host_arithmetic_matches_the_model(gm, blocks, curve):
    c = gm.CURVES[curve]
    r, g = c.r, c.fr_mult_gen
    get = lambda tag: [l[1:] for l in blocks[curve] if l[0] == tag]
    assert [int(x[1]) for x in get("div")] == [fm.next_divisor(n, r) for n in range(1, 17)]
    assert int(get("root6")[0][0], 16) == fm.ith_root_one(6, r, g)
    ts = [fm.next_divisor(len(p), r) for p in PACKS]
    assert [int(x[0], 16) for x in get("ext")] == [x for s, t in zip(POINTS, ts) for x in fm.extend_set(s, t, r, g)]
    w, _, _, _ = fm.shortcut_batch_open(PACKS, POINTS, 12345, 999, r, g)
    _, claimed, folded, _ = fm.reference_batch_open(PACKS, POINTS, 12345, 999, r, g)
    assert [int(x[0], 16) for x in get("claimed")] == [v for rows in claimed for row in rows for v in row]
    assert [int(x[0], 16) for x in get("folded")] == [v for f in folded for v in f]
    plan = get("plan")[0]  # rc, maxfold, the true length of w, remainders, extended points
    assert plan[0] == "0" and int(plan[2]) == max(t * max(len(q) for q in p) for p, t in zip(PACKS, ts))
    assert int(plan[4]) == len(sm.strip(w)) and int(plan[6]) == 2 * 2 + 5 * 1 and int(plan[8]) == 2 * 2 + 6 * 1
    assert [int(v) for v in get("tables")[0]] == [0, 3, 3, 2, 5, 1, 6, 0, 6, 2, 8, 4, 12, 1, 2, 0, 2, 6, 2, 5]
    # 1 and -1 share an orbit for t = 2; z = 0 with t = 2; a key one point short of the folded size condition, then exact
    assert [get(k)[0][0] for k in ("equal", "zero_t2", "size_short", "size_exact")] == ["4", "4", "4", "0"]
    # singleton form: every polynomial its own group with t = 1
    w, claimed = sm.chain_open_w(S_POLYS, S_POINTS, 12345, r)
    assert claimed == [[sm.eval_poly(f, x, r) for x in s] for f, s in zip(S_POLYS, S_POINTS)]
    plan = get("s_plan")[0]  # rc, maxfold, the true length of w, remainders
    assert plan[0] == "0" and int(plan[2]) == max(len(f) for f in S_POLYS)
    assert int(plan[4]) == len(sm.strip(w)) == 1 and int(plan[6]) == sum(len(s) for s in S_POINTS)
    assert [int(v) for v in get("s_tables")[0]] == [0, 3, 3, 2, 5, 1, 1, 0, 1, 1, 1, 1, 1, 2, 1]
    assert [int(x[0], 16) for x in get("s_claimed")] == sm.flatten(claimed)
    # a point twice in one set; one point in two sets; a key one base short of max_size + sum m_i - 1, then exact
    assert [get(k)[0][0] for k in ("s_equal", "s_shared", "s_size_short", "s_size_exact")] == ["4", "0", "4", "0"]
