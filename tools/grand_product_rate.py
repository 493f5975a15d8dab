#!/usr/bin/env python3
"""The batched grand-product argument on one MI355X, in one process (warm-up first, then the forms alternate rep by rep; medians of
--reps with the spread), end to end through the ctypes face, at the shapes of DESIGN.md s7g -- 1024 x 2^10, 256 x 2^14, 16 x 2^20
and 1 x 2^24 -- over device-resident random columns:
  (A) prover      zigz_dev_grand_product_prove_batch (Fiat-Shamir);
  (B) assembled   what a caller could assemble from this same build without the prover entry: zigz_dev_product_layers_batch into
                  its own buffers, then ONE zigz_dev_sumcheck_prove_zerocheck_batch call per layer j = 2 .. v - 1 over the halves of
                  layer j + 1 of every instance, at fixed challenges (the taus and round challenges of (A)'s proof, so that the
                  two forms write the same rounds: checked here).  Layers 0 and 1 are left out of (B) -- layer 0 has no rounds, and
                  layer 1's second table starts 8 bytes into a 16-byte vector, which the device form does not take --, and so is the
                  transcript a caller would have to run between the calls: (B) is timed in its favour.
The parent commit cannot state a grand product at all, so (B) is the only comparable route.  Condition at the two large shapes:
(A)'s median is not above (B)'s by more than the sum of the two spreads.

Also, at 1 x 2^24: zigz_dev_product_layers_batch alone, timed until the stream has drained, with the bytes its k_gp_layers launches
move (a pass of L levels from layer J reads 4 * 2^J bytes and writes 4 * 2^J * (1 - 2^-L)) and, for comparison in the same
process, zigz_dev_eq_table_batch at the same size (4 N written bytes; tools/eq_table_rate.py).

    python tools/grand_product_rate.py [--reps R] [--quick | --trees-only]      (prints one JSON object)

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
JUDGED = ("16x2^20", "1x2^24")
TRACED = "16x2^20"
TOP_LOG2 = 11


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(xs.min()), 4), "max_ms": round(float(xs.max()), 4)}


def layer_pass_bytes(v):
    """(read, written) bytes of the k_gp_layers launches of one column of 2^v words, and the passes"""
    rd = wr = passes = 0
    J = v
    while J > TOP_LOG2:
        L = min(3, J - TOP_LOG2)
        rd += 4 << J
        wr += (4 << J) - (4 << (J - L))
        J -= L
        passes += 1
    return rd, wr, passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form at 16 x 2^20 only (for a kernel trace)")
    ap.add_argument("--trees-only", action="store_true",
                    help="the layers entry and the eq table entry alone at 1 x 2^24, --reps calls of each behind two warm-ups (for a kernel trace)")
    a = ap.parse_args()
    reps = 2 if a.quick else a.reps
    import zigz_amd
    from zigz_amd import hip

    P = hip.P
    ctx = zigz_amd.Context(0)
    if a.trees_only:
        v, n = 24, 1 << 24
        rng = np.random.default_rng(13)
        bufs = [ctx.dev_alloc(4 * n) for _ in range(3)]
        ctx.upload(rng.integers(1, P, size=n, dtype=np.uint64), bufs[0])
        tau = [rng.integers(0, P, size=v, dtype=np.uint64)]
        for _ in range(2 + reps):
            ctx.dev_product_layers_batch([bufs[0]], [n], [bufs[1]])
            ctx.dev_eq_table_batch([bufs[2]], [n], tau)
            ctx.synchronize()
        rd, wr, passes = layer_pass_bytes(v)
        print(json.dumps({"calls_of_each": 2 + reps, "passes": passes, "k_gp_layers_bytes_per_call": rd + wr, "k_eq_batch_expand_bytes_per_call": 4 * n}))
        for b in bufs:
            ctx.dev_free(b)
        ctx.close()
        return
    out = {"reps": reps, "statement": "prod_x A[x], layered product tree, one transcript per instance", "shapes": {}}
    rng = np.random.default_rng(13)
    term = [(1, (0, 1))]
    for name, logs in SHAPES:
        if a.quick and name != TRACED:
            continue
        ns = [1 << v for v in logs]
        v = logs[0]
        total = int(sum(ns))
        offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        cols_h = rng.integers(1, P, size=total, dtype=np.uint64)
        d_cols, d_trees = ctx.dev_alloc(total * 4), ctx.dev_alloc(total * 4)
        ctx.upload(cols_h, d_cols)
        cols = [d_cols + 4 * int(o) for o in offs[:-1]]
        trees = [d_trees + 4 * int(o) for o in offs[:-1]]

        def prover():
            return ctx.dev_grand_product_prove_batch(cols, ns)

        proofs = prover()
        # (B)'s calls: per layer the instances, taus and fixed challenges from (A)'s proofs
        calls = []
        for j in range(2, v):
            inst, chal = [], []
            for (_, evals, _, points, chs, _, _), c, t, n in zip(proofs, cols, trees, ns):
                q = [int(x) for x in points[(j - 1) * (j - 2) // 2: (j - 1) * (j - 2) // 2 + j - 1]][::-1]
                nxt = c if j + 1 == v else t + 4 * (n - (2 << (j + 1)))
                inst.append(([nxt, nxt + 4 * (1 << j)], term, q + [int(chs[j - 1])]))
                chal.append(points[j * (j - 1) // 2: j * (j - 1) // 2 + j])
            calls.append((inst, [1 << j] * len(ns), chal))

        def assembled():
            ctx.dev_product_layers_batch(cols, ns, trees)
            return [ctx.dev_sumcheck_prove_zerocheck_batch(*c) for c in calls]

        res = {"words": total}
        layers = assembled()
        res["same_round_words"] = all(np.array_equal(got[1], p[2][2 * j * (j - 1): 2 * j * (j + 1)])
                                      for j, call in zip(range(2, v), layers) for got, p in zip(call, proofs))
        forms = [("prover", prover, []), ("assembled", assembled, [])]
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
        pa, pb = res["prover"], res["assembled"]
        res["prover_over_assembled"] = round(pa["median_ms"] / pb["median_ms"], 3)
        if name in JUDGED:
            res["condition_holds"] = bool(pa["median_ms"] <= pb["median_ms"] + (pa["max_ms"] - pa["min_ms"]) + (pb["max_ms"] - pb["min_ms"]))
        if name == "1x2^24" and not a.quick:
            eq_out = ctx.dev_alloc(total * 4)
            tau = [rng.integers(0, P, size=v, dtype=np.uint64)]

            def trees_alone():
                ctx.dev_product_layers_batch(cols, ns, trees)
                ctx.synchronize()

            def eq_table():
                ctx.dev_eq_table_batch([eq_out], ns, tau)
                ctx.synchronize()

            acc = {"layers": [], "eq_table": []}
            for _ in range(2):
                trees_alone()
                eq_table()
            for _ in range(reps):
                for label, f in (("layers", trees_alone), ("eq_table", eq_table)):
                    t0 = time.perf_counter()
                    f()
                    acc[label].append(time.perf_counter() - t0)
            rd, wr, passes = layer_pass_bytes(v)
            lt, et = stats(acc["layers"]), stats(acc["eq_table"])
            res["layers_entry"] = dict(lt, passes=passes, k_gp_layers_bytes_read=rd, k_gp_layers_bytes_written=wr,
                                       end_to_end_TBps=round((rd + wr) / (lt["median_ms"] * 1e-3) / 1e12, 3))
            res["eq_table_entry"] = dict(et, bytes_written=4 * total, end_to_end_TBps=round(4 * total / (et["median_ms"] * 1e-3) / 1e12, 3))
            ctx.dev_free(eq_out)
        out["shapes"][name] = res
        ctx.dev_free(d_cols)
        ctx.dev_free(d_trees)
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
