"""ToLagrangeG1 on one GPU: python tools/bench_to_lagrange.py [--out profiles/to_lagrange.json] [--reps R] [--trace CSV]
                                                             [--rows bn254:16,bn254:20,...]

Per (curve, n): host in / host out (kzg.ToLagrangeG1, as the Go drop-in passes it) and device in / device out
(to_lagrange_device over torch tensors), host clock around blocking calls, median of R after one warm-up. Each row
carries the field-product count of the chosen method (gmsm_group_fft.h: GLV joint walk, 1/n folded into stage 0, twiddle 1
skipped) and its bound against the measured product rate of the coordinate field (profiles/peaks_r06.json).

Kernel times come from a run of its own under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d DIR -o lag -- python tools/bench_to_lagrange.py --reps 1 --out /dev/null
then --trace TRACE (the run's lag_results.db, or a kernel_trace.csv of -f csv) attributes the dispatches of the traced
run's last call of every row to the stage classes (stage 0, the other per-lane stages 1-5, the wave-uniform stages 6+,
load + twiddles + normalisation) and adds frac_of_measured = product bound / stage kernel time: on a timing run, or
with --attach-to JSON on a record written before (no GPU needed)."""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gm = importlib.import_module("gnark-crypto_amd")

PEAKS = json.load(open(os.path.join(ROOT, "profiles", "peaks_r06.json")))
PRODUCT_RATE = {c: PEAKS[f"{c}_fp_mul_unsigned"] for c in ("bn254", "bls12_381", "bw6_761")}
FP_PARAMS = {"bn254": "bn254_fp_params", "bls12_381": "bls12_381_fp_params", "bw6_761": "bw6_761_fp_params"}
GLV_BITS = {"bn254": 127, "bls12_381": 128, "bw6_761": 190}
ROWS = [("bn254", 16), ("bn254", 20), ("bn254", 22), ("bls12_381", 20), ("bw6_761", 18)]
# field products of the group law in gmsm_curveu.h (a product-sum Y3 counted as two)
DBL, ADD, TABLE = 9, 14, 15  # double_u, add_u, phi + the table's P1 + P2
UNIFORM_FROM = 6


def products(curve, logn):
    """expected products of one call, per stage class: butterflies (2 additions) + twiddle products (table + walk; one
    doubling per bit, an addition where the digit pair is not (0, 0): 3/4 of the bits in a wave-uniform stage, every bit
    in a per-lane stage - the wave adds when any lane does)"""
    n, b = 1 << logn, GLV_BITS[curve]
    half = n // 2
    per = {"stage0": 0, "per_lane_1_5": 0, "uniform_6_up": 0}
    for s in range(logn):
        muls = n if s == 0 else half - (half >> s)  # stage s > 0: the butterflies at i = 0 skip (twiddle 1)
        add_frac = 1.0 if s < UNIFORM_FROM else 0.75
        p = 2 * ADD * half + muls * (TABLE + b * DBL + b * add_frac * ADD)
        per["stage0" if s == 0 else "per_lane_1_5" if s < UNIFORM_FROM else "uniform_6_up"] += p
    return per


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def row(curve, logn, reps):
    n = 1 << logn
    g = gm.G1Affine(curve)
    rng = np.random.default_rng([0x1A6, logn])
    # distinct points: repeated ones would cancel in the butterflies (a - b = infinity) and skip the twiddle products
    pts = g.generate_points(n, int(rng.integers(1, 2**62)), int(rng.integers(1, 2**62)))
    out = {"curve": curve, "group": "g1", "logn": logn, "n": n}
    out["host_ms"] = timed(lambda: gm.kzg.ToLagrangeG1(curve, pts), reps)
    stream = torch.cuda.current_stream().cuda_stream
    d_in = torch.from_numpy(pts.view(np.int64).copy()).cuda()
    d_out = torch.empty_like(d_in)
    out["device_ms"] = timed(lambda: gm.kzg.to_lagrange_device(curve, d_in.data_ptr(), n, d_out.data_ptr(), stream), reps)
    per = products(curve, logn)
    total = sum(per.values())
    rate = PRODUCT_RATE[curve]
    out["products"] = {"per_class": per, "total": total, "rate_per_s": rate, "bound_ms": total / rate * 1e3,
                       "method": "GLV joint binary walk, table in HBM, 1/n folded into stage 0, twiddle 1 skipped"}
    out["bound_over_device_ms"] = out["products"]["bound_ms"] / out["device_ms"]
    del d_in, d_out
    gm.trim(0)
    return out


def dispatches(path):
    """(name, start ns, end ns) of every kernel dispatch of a traced run, in start order"""
    if path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(path)
        recs = [{"Kernel_Name": n, "Start_Timestamp": a, "End_Timestamp": b} for n, a, b in db.execute("select name, start, end from kernels")]
    else:
        with open(path) as f:
            recs = list(csv.DictReader(f))
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    return recs


def kernel_times(path, rows):
    """dispatches of the traced run -> per row, the last call's kernel times (ms) by stage class"""
    recs = dispatches(path)
    calls = {}  # (curve, logn) -> list of calls, each a list of (name, ms)
    cur = None
    for r in recs:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "k_group_fft_load" in name:
            cur = [(name, ms)]
            continue
        if cur is None:
            continue
        if "k_group_fft_" in name or ("k_batch_normalize" in name and cur):
            cur.append((name, ms))
            if "k_batch_normalize" in name:
                curve = next(c for c, p in FP_PARAMS.items() if p in cur[0][0])
                logn = sum("k_group_fft_stage" in k for k, _ in cur)
                calls.setdefault((curve, logn), []).append(cur)
                cur = None
    out = {}
    for curve, logn in rows:
        if (curve, logn) not in calls:
            continue
        call = calls[(curve, logn)][-1]
        stages = [ms for k, ms in call if "k_group_fft_stage" in k]
        other = sum(ms for k, ms in call if "k_group_fft_stage" not in k)
        out[(curve, logn)] = {"stage0_ms": stages[0], "per_lane_1_5_ms": sum(stages[1:UNIFORM_FROM]),
                              "uniform_6_up_ms": sum(stages[UNIFORM_FROM:]), "stages_ms": sum(stages),
                              "load_twiddles_normalize_ms": other, "per_stage_ms": stages}
    return out


def attach(res, trace):
    kt = kernel_times(trace, [(r["curve"], r["logn"]) for r in res])
    for r in res:
        k = kt.get((r["curve"], r["logn"]))
        if not k:
            continue
        r["kernels"] = k
        p = r["products"]["per_class"]
        rate = r["products"]["rate_per_s"]
        r["frac_of_measured"] = {
            "stages": r["products"]["total"] / rate * 1e3 / k["stages_ms"],
            "stage0": p["stage0"] / rate * 1e3 / k["stage0_ms"],
            "per_lane_1_5": p["per_lane_1_5"] / rate * 1e3 / k["per_lane_1_5_ms"] if k["per_lane_1_5_ms"] else None,
            "uniform_6_up": p["uniform_6_up"] / rate * 1e3 / k["uniform_6_up_ms"] if k["uniform_6_up_ms"] else None,
            "note": "expected field products of the class / its traced kernel time, against the measured product rate"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "to_lagrange.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--rows", default=None)
    ap.add_argument("--attach-to", default=None, help="add the kernel times of --trace to this record, no GPU run")
    a = ap.parse_args()
    if a.attach_to:
        rec = json.load(open(a.attach_to))
        attach(rec["rows"], a.trace)
        rec["trace"] = os.path.basename(a.trace)
        with open(a.attach_to, "w") as f:
            json.dump(rec, f, indent=1)
        return
    rows = ROWS if not a.rows else [(x.split(":")[0], int(x.split(":")[1])) for x in a.rows.split(",")]
    res = []
    for curve, logn in rows:
        r = row(curve, logn, a.reps)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.trace:
        attach(res, a.trace)
    rec = {"tool": "tools/bench_to_lagrange.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": res,
           "lib": os.environ.get("GMSM_LIB", "gnark-crypto_amd/csrc/libgmsm.so")}
    if a.out != "/dev/null":
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
