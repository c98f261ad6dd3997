#!/usr/bin/env python3
"""GMSM_OPT_REDUCE_TAIL 1 (device ladder) against 2 (host planes) in ONE process on the same resident inputs: `calls` MultiExp
calls per form, interleaved in blocks of `block`, wall time per call (median and mean over the calls) and the share of the
calls that really took the host form (gmsm_debug_plane_runs: shapes the planes do not cover fall back to the ladder).
Also the host fold alone (no device): microseconds per fold of the ladder's window totals and of the plane sums.
usage: python tools/reduce_tail_ab.py [curve group] [--logns=16,20,22,24] [--calls=50] [--block=10] [--out=FILE.json]"""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_fold_times(g, c=16, log2L=3, nblocks1=64, reps=300):
    """us per gmsm_fold_windows and per gmsm_debug_fold_planes over finite values with zz != 1 (what the device hands out):
    (x, y) -> (x l^2, y l^3, l^2, l^3). Groups over Fp."""
    nwin = g.num_windows(c)
    NP = 7 + (nblocks1 - 1).bit_length()
    pts = g.generate_points(nwin * NP, 3, 5)
    L, p = g.coord_limbs, g.curve.p
    Rm = 1 << (64 * L)
    Rinv = pow(Rm, -1, p)
    to_int = lambda limbs: sum(int(v) << (64 * i) for i, v in enumerate(limbs)) * Rinv % p
    to_limbs = lambda v: [((v * Rm % p) >> (64 * i)) & (2**64 - 1) for i in range(L)]
    planes = np.zeros((nwin * NP, g.xyzz_limbs), dtype=np.uint64)
    for i in range(nwin * NP):
        lam = 3 + 2 * i
        x, y = to_int(pts[i, :L]), to_int(pts[i, L:2 * L])
        planes[i] = to_limbs(x * lam**2 % p) + to_limbs(y * lam**3 % p) + to_limbs(lam**2 % p) + to_limbs(lam**3 % p)
    totals = planes[:nwin].copy()
    out = {}
    for name, fn in (("fold_windows_us", lambda: g.fold_windows(totals, c)),
                     ("fold_planes_us", lambda: g.fold_planes(planes, c, nwin, log2L, nblocks1))):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out[name] = round((time.perf_counter() - t0) / reps * 1e6, 2)
    extra = nwin * (NP - 1)
    out.update(c=c, nwin=nwin, planes_per_window=NP, log2L=log2L, extra_additions=extra,
               extra_us_per_addition=round((out["fold_planes_us"] - out["fold_windows_us"]) / extra, 3))
    return out


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    curve, group = (argv + ["bn254", "g1"])[:2]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    logns = [int(x) for x in opt.get("logns", "16,20,22,24").split(",")]
    calls, block = int(opt.get("calls", 50)), int(opt.get("block", 10))
    gm = importlib.import_module("gnark-crypto_amd")
    g = (gm.G1Jac if group == "g1" else gm.G2Jac)(curve)
    lib = gm._lib.load()
    res = {"curve": curve, "group": group, "calls_per_form": calls, "block": block, "rows": []}
    if group == "g1":
        res["host_fold"] = host_fold_times(g)
        print(json.dumps(res["host_fold"]), file=sys.stderr, flush=True)
    if "--host-only" not in sys.argv:
        import torch
        import bench
        assert lib.gmsm_set_device(0) == 0
        torch.cuda.set_device(0)
        for logn in logns:
            n = 1 << logn
            pts, sc = bench.headline_inputs(g, logn)
            d_pts = torch.from_numpy(pts.view(np.int64)).cuda()
            d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
            call = lambda: g.multiexp_device(d_pts.data_ptr(), d_sc.data_ptr(), n)
            times = {1: [], 2: []}
            planes = {1: 0, 2: 0}
            for tail in (1, 2):  # warm both forms: allocations, LDS attributes
                with gm.options(reduce_tail=tail):
                    ref = call() if tail == 1 else ref
                    assert (g.jac_to_affine(call()) == g.jac_to_affine(ref)).all()
            done = 0
            while done < calls:
                for tail in (1, 2):
                    with gm.options(reduce_tail=tail):
                        before = int(lib.gmsm_debug_plane_runs())
                        for _ in range(min(block, calls - done)):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            call()
                            times[tail].append((time.perf_counter() - t0) * 1e3)
                        planes[tail] += int(lib.gmsm_debug_plane_runs()) - before
                done += block
            row = {"logn": logn, "window_bits": g.default_window_bits(n),
                   "ladder_ms_median": round(statistics.median(times[1]), 4), "planes_ms_median": round(statistics.median(times[2]), 4),
                   "ladder_ms_mean": round(statistics.fmean(times[1]), 4), "planes_ms_mean": round(statistics.fmean(times[2]), 4),
                   "plane_runs": planes[2], "plane_runs_under_ladder": planes[1]}
            row["delta_us_median"] = round((row["planes_ms_median"] - row["ladder_ms_median"]) * 1e3, 1)
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del d_pts, d_sc
            torch.cuda.empty_cache()
    text = json.dumps(res)
    if "out" in opt:
        with open(opt["out"], "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
