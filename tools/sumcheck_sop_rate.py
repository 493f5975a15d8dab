#!/usr/bin/env python3
"""The batched sum-of-products sumcheck prover on one MI355X, in one process (warm-up first, then the forms alternate rep by rep;
medians of --reps with the spread), end to end through the ctypes face, at the shapes of DESIGN.md s7g -- 1024 x 2^10, 256 x 2^14,
16 x 2^20 and 1 x 2^24.  The statement is the zero-check of a*b - c = 0 over device-resident tables eq, a, b, c:
  (A) sop        zigz_dev_sumcheck_prove_sop_batch, per constraint a pool of 4 and the terms (1; eq a b), (p - 1; eq c);
  (B) per_term   what the product entry offers: 2 instances per constraint, {eq, a, b} and {eq, c}, in one call
                 (zigz_dev_sumcheck_prove_product_batch; T transcripts and T points, so not one proof of the constraint).
Fiat-Shamir challenges differ between the two, so the proofs are not compared here (tests/test_gpu_sumcheck_sop.py does, under
fixed challenges); (A)'s claimed sums are checked to be 0 because c = a*b.

    python tools/sumcheck_sop_rate.py [--reps R] [--quick]      (prints one JSON object)
    python tools/sumcheck_sop_rate.py --kernel-times DB         (prints one JSON object)

--quick: two reps of each form at 16 x 2^20 only, and of the product entry at d = 3 over {eq, a, b} alone, for a kernel trace
(rocprofv3 --kernel-trace --stats in a run of its own, no counters).
--kernel-times reads that run's database: k_sop_bind at the first bound round of 16 x 2^20 (the launches with 16 x 2^20 / 8192
workgroups) against the bytes it moves -- every pool table's n words read and n / 2 written, 16 x 12 x M x n / 2 -- and
k_product_bind at d = 3 from the same run (the launches with as many workgroups that do not follow one of twice as many: form
(B) has twice as many in its first bound round and as many in its second).
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
TRACED = "16x2^20"
POOL = 4


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(xs.min()), 4), "max_ms": round(float(xs.max()), 4)}


def kernel_times(db):
    """the bind passes' kernel times at the first bound round of 16 x 2^20 from a rocprofv3 --kernel-trace database"""
    import sqlite3
    logs = dict(SHAPES)[TRACED]
    wgs = sum(((1 << v) + 8191) // 8192 for v in logs)
    n = 1 << logs[0]
    out = {}
    for kernel, tables in (("k_sop_bind", POOL), ("k_product_bind", 3)):
        rows = sqlite3.connect(db).execute(
            "select end - start, grid_x / 256 from kernels where name like ? order by start", (f"%{kernel}%",)).fetchall()
        # the first bound round of a call over 16 tables: `wgs` workgroups, and not the launch behind one of twice as many (form
        # (B)'s second bound round has as many workgroups as the 16-instance forms' first)
        us = sorted(t / 1e3 for x, (t, g) in enumerate(rows) if g == wgs and (x == 0 or rows[x - 1][1] != 2 * wgs))
        if not us:
            out[kernel] = {"launches": 0}
            continue
        med = us[len(us) // 2]
        moved = len(logs) * 12 * tables * (n // 2)  # 4 n read + 2 n written per table
        out[kernel] = {"launches": len(us), "tables": tables, "median_us": round(med, 2), "min_us": round(us[0], 2),
                       "max_us": round(us[-1], 2), "bytes_moved": moved, "TBps_of_bytes_moved": round(moved / med / 1e6, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form at 16 x 2^20 only (for a kernel trace)")
    ap.add_argument("--kernel-times", metavar="DB", help="read the bind passes' kernel times from a rocprofv3 database")
    a = ap.parse_args()
    if a.kernel_times:
        print(json.dumps({"first_bound_round_16x2^20": kernel_times(a.kernel_times)}))
        return
    reps = 2 if a.quick else a.reps
    import zigz_amd
    from zigz_amd import hip

    P = hip.P
    ctx = zigz_amd.Context(0)
    out = {"reps": reps, "statement": "sum_x eq(tau, x) (a(x) b(x) - c(x)), c = a*b", "shapes": {}}
    rng = np.random.default_rng(12)
    terms = [(1, (0, 1, 2)), (P - 1, (0, 3))]
    for name, logs in SHAPES:
        if a.quick and name != TRACED:
            continue
        ns = [1 << v for v in logs]
        total = int(sum(ns))
        offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        ta, tb = (rng.integers(0, P, size=total, dtype=np.uint64) for _ in range(2))
        bases = [ctx.dev_alloc(total * 4) for _ in range(POOL)]  # table j of every instance in buffer j (16-byte aligned: n >= 1024)
        ctx.dev_eq_table_batch([bases[0] + 4 * int(o) for o in offs[:-1]], ns, [rng.integers(0, P, size=v, dtype=np.uint64) for v in logs])
        for b, t in zip(bases[1:], (ta, tb, (ta * tb) % np.uint64(P))):
            ctx.upload(t, b)
        pools = [[b + 4 * int(o) for b in bases] for o in offs[:-1]]
        sop_inst = [(p, terms) for p in pools]
        per_term = [f for p in pools for f in (p[:3], [p[0], p[3]])]
        per_term_ns = [n for n in ns for _ in range(2)]
        cubic = [p[:3] for p in pools]

        def sop():
            return ctx.dev_sumcheck_prove_sop_batch(sop_inst, ns)

        def product():
            return ctx.dev_sumcheck_prove_product_batch(per_term, per_term_ns)

        def product_d3():
            return ctx.dev_sumcheck_prove_product_batch(cubic, ns)

        forms = [("sop", sop, []), ("per_term", product, [])] + ([("product_d3_alone", product_d3, [])] if a.quick else [])
        res = {"elements_per_table": total, "claimed_sums_zero": all(p[0] == 0 for p in sop())}
        for _ in range(2):
            for _, form, _acc in forms:
                form()
        for _ in range(reps):
            for _, form, acc in forms:
                t0 = time.perf_counter()
                form()
                acc.append(time.perf_counter() - t0)
        for label, _, acc in forms:
            res[label] = stats(acc)
        res["sop_over_per_term"] = round(res["sop"]["median_ms"] / res["per_term"]["median_ms"], 3)
        out["shapes"][name] = res
        for b in bases:
            ctx.dev_free(b)
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
