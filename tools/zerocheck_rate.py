#!/usr/bin/env python3
"""The zero-check sumcheck with the eq factor in closed form on one MI355X, in one process (warm-up first, then the forms alternate
rep by rep; medians of --reps with the spread), end to end through the ctypes face, at the shapes of DESIGN.md s7g -- 1024 x 2^10,
256 x 2^14, 16 x 2^20 and 1 x 2^24.  The statement is the zero-check of a*b - c = 0 over device-resident tables a, b, c and a tau
per instance:
  (A) closed       zigz_dev_sumcheck_prove_zerocheck_batch, per constraint a pool of 3 and the terms (1; a b), (p - 1; c);
  (B) table_route  what the library offered before: zigz_dev_eq_table_batch into a fourth buffer, then
                   zigz_dev_sumcheck_prove_sop_batch with a pool of 4 and the terms (1; a b eq), (p - 1; c eq) -- both calls timed;
  (C) degree4      eq * a * b * c, a pool of 3 and one term, through (A)'s entry: recorded with no counterpart (nothing else proves it).
(A) and (B) write the same proof (tests/test_gpu_zerocheck_closed.py compares them word for word); here their claimed sums are
checked to be 0 because c = a*b, and their round words to be equal.

    python tools/zerocheck_rate.py [--reps R] [--quick] [--table-route-only]      (prints one JSON object)

--table-route-only: (B) alone, for a build that does not have (A)'s entry (the parent commit: this tool does not touch (B)'s code).
--quick: two reps of each form at 16 x 2^20 only, for a kernel trace (rocprofv3 --kernel-trace --stats in a run of its own, no
counters).
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


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(xs.min()), 4), "max_ms": round(float(xs.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form at 16 x 2^20 only (for a kernel trace)")
    ap.add_argument("--table-route-only", action="store_true", help="time (B) alone: a build without the closed-form entry")
    a = ap.parse_args()
    reps = 2 if a.quick else a.reps
    import zigz_amd
    from zigz_amd import hip

    P = hip.P
    ctx = zigz_amd.Context(0)
    out = {"reps": reps, "statement": "sum_x eq(tau, x) (a(x) b(x) - c(x)), c = a*b", "table_route_only": a.table_route_only, "shapes": {}}
    rng = np.random.default_rng(12)
    closed_terms = [(1, (0, 1)), (P - 1, (2,))]
    table_terms = [(1, (0, 1, 3)), (P - 1, (2, 3))]
    for name, logs in SHAPES:
        if a.quick and name != TRACED:
            continue
        ns = [1 << v for v in logs]
        total = int(sum(ns))
        offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        ta, tb = (rng.integers(0, P, size=total, dtype=np.uint64) for _ in range(2))
        taus = [rng.integers(0, P, size=v, dtype=np.uint64) for v in logs]
        bases = [ctx.dev_alloc(total * 4) for _ in range(4)]  # table j of every instance in buffer j (16-byte aligned: n >= 1024)
        for b, t in zip(bases[:3], (ta, tb, (ta * tb) % np.uint64(P))):
            ctx.upload(t, b)
        pools = [[b + 4 * int(o) for b in bases] for o in offs[:-1]]
        eq_out = [p[3] for p in pools]
        table_inst = [(p, table_terms) for p in pools]

        def table_route():
            ctx.dev_eq_table_batch(eq_out, ns, taus)
            return ctx.dev_sumcheck_prove_sop_batch(table_inst, ns)

        forms = [("table_route", table_route, [])]
        res = {"elements_per_table": total}
        if not a.table_route_only:
            closed_inst = [(p[:3], closed_terms, tau) for p, tau in zip(pools, taus)]
            quartic_inst = [(p[:3], [(1, (0, 1, 2))], tau) for p, tau in zip(pools, taus)]

            def closed():
                return ctx.dev_sumcheck_prove_zerocheck_batch(closed_inst, ns)

            def degree4():
                return ctx.dev_sumcheck_prove_zerocheck_batch(quartic_inst, ns)

            forms = [("closed", closed, []), ("table_route", table_route, []), ("degree4", degree4, [])]
            pa, pb = closed(), table_route()
            res["claimed_sums_zero"] = all(p[0] == 0 for p in pa) and all(p[0] == 0 for p in pb)
            res["same_round_words"] = all(np.array_equal(x[1], y[1]) for x, y in zip(pa, pb))
        else:
            res["claimed_sums_zero"] = all(p[0] == 0 for p in table_route())
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
        if not a.table_route_only:
            res["closed_over_table_route"] = round(res["closed"]["median_ms"] / res["table_route"]["median_ms"], 3)
        out["shapes"][name] = res
        for b in bases:
            ctx.dev_free(b)
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
