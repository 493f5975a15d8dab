#!/usr/bin/env python3
"""The batched product sumcheck prover on one MI355X, in one process (warm-up first, then the forms alternate rep by rep; medians
of --reps with the spread): zigz_dev_sumcheck_prove_product_batch over device-resident tables for d = 1, 2, 3 at the shapes of
DESIGN.md s7b -- 1024 x 2^10, 256 x 2^14, 16 x 2^20 and 1 x 2^24 -- end to end through the ctypes face, and for d = 1 the ratio to
zigz_dev_sumcheck_prove_batch (the radix schedule) over the same tables in the same run: what one data pass per round costs
against several rounds per pass.  Every d = 1 proof is checked against the linear prover's, bytes-equal.

    python tools/sumcheck_product_rate.py [--reps R] [--quick]      (prints one JSON object)
    python tools/sumcheck_product_rate.py --kernel-times DB         (prints one JSON object)

--quick: two reps of each form at 16 x 2^20 only, for a kernel trace (rocprofv3 --kernel-trace --stats in a run of its own, no
counters; 1 x 2^24 is left out because its first bound round has the same workgroup count).
--kernel-times reads that run's database: the kernel time of k_product_bind at the first bound round of 16 x 2^20 (the launches
with 16 x 2^20 / 8192 workgroups; the tool runs d = 1, 2, 3 in that order with the same number of calls each, so the launches in
time order fall into thirds) against the bytes that round moves -- every factor's n words read and n / 2 written, 6 n bytes per
factor -- at the 8 TB/s the README prices k_radix_fold with.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1024x2^10", [10] * 1024), ("256x2^14", [14] * 256), ("16x2^20", [20] * 16), ("1x2^24", [24])]
DEGREES = (1, 2, 3)
TRACED = "16x2^20"


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(xs.min()), 4), "max_ms": round(float(xs.max()), 4)}


def kernel_times(db):
    """k_product_bind's kernel time at the first bound round of 16 x 2^20, per degree, from a rocprofv3 --kernel-trace database"""
    import sqlite3
    logs = dict(SHAPES)[TRACED]
    wgs = sum(((1 << v) + 8191) // 8192 for v in logs)
    n = 1 << logs[0]
    rows = sqlite3.connect(db).execute(
        "select start, end - start from kernels where name like '%k_product_bind%' and grid_x / 256 = ? order by start", (wgs,)).fetchall()
    out = {"launches": len(rows)}
    if not rows or len(rows) % len(DEGREES):
        return out
    per = len(rows) // len(DEGREES)
    for x, d in enumerate(DEGREES):
        us = sorted(t / 1e3 for _, t in rows[x * per: (x + 1) * per])
        med = us[len(us) // 2]
        moved = len(logs) * d * 6 * n  # 4 n read + 2 n written per factor
        out[f"d{d}"] = {"launches": len(us), "median_us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                        "bytes_moved_6dn": moved, "hbm_bound_us_at_8TBps": round(moved / 8e12 * 1e6, 2),
                        "TBps_of_bytes_moved": round(moved / med / 1e6, 3),
                        # per bound WORD the pass moves 12 bytes; priced at 6 per bound word, d * 6 * (n / 2), the bound halves
                        "hbm_bound_us_of_d_6_half_n_at_8TBps": round(moved / 2 / 8e12 * 1e6, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form at 16 x 2^20 only (for a kernel trace)")
    ap.add_argument("--kernel-times", metavar="DB", help="read k_product_bind's kernel times from a rocprofv3 database")
    a = ap.parse_args()
    if a.kernel_times:
        print(json.dumps({"k_product_bind_first_bound_round_16x2^20": kernel_times(a.kernel_times)}))
        return
    reps = 2 if a.quick else a.reps
    import zigz_amd
    from zigz_amd import hip

    P = hip.P
    ctx = zigz_amd.Context(0)
    out = {"reps": reps, "launches_per_round": {"launches": 2, "copies": 1}, "shapes": {}}
    rng = np.random.default_rng(11)
    for name, logs in SHAPES:
        if a.quick and name != TRACED:
            continue
        ns = [1 << v for v in logs]
        total = int(sum(ns))
        bases = []
        for _ in range(max(DEGREES)):  # factor j of every instance in buffer j (every table 16-byte aligned: n >= 1024)
            b = ctx.dev_alloc(total * 4)
            ctx.upload(rng.integers(0, P, size=total, dtype=np.uint64), b)
            bases.append(b)
        offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        res = {"elements_per_factor": total}
        linear_ptrs = [bases[0] + 4 * int(o) for o in offs[:-1]]
        for d in DEGREES:
            ptrs = [[bases[j] + 4 * int(o) for j in range(d)] for o in offs[:-1]]

            def product():
                return ctx.dev_sumcheck_prove_product_batch(ptrs, ns)

            def linear():
                return ctx.dev_sumcheck_prove_batch(linear_ptrs, ns)

            forms = [(product, [])] + ([(linear, [])] if d == 1 else [])
            first = product()
            if d == 1:
                res["d1_bytes_equal_to_the_linear_prover"] = all(
                    p[1].tobytes() == l[0].tobytes() and p[2].tobytes() == l[1].tobytes() and p[4] == l[2]
                    for p, l in zip(first, linear()))
            for _ in range(2):
                for form, _acc in forms:
                    form()
            for _ in range(reps):
                for form, acc in forms:
                    t0 = time.perf_counter()
                    form()
                    acc.append(time.perf_counter() - t0)
            res[f"d{d}"] = stats(forms[0][1])
            if d == 1:
                res["linear_radix"] = stats(forms[1][1])
                res["d1_over_linear_radix"] = round(res["d1"]["median_ms"] / res["linear_radix"]["median_ms"], 2)
        out["shapes"][name] = res
        for b in bases:
            ctx.dev_free(b)
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
