#!/usr/bin/env python3
"""One call of every entry that runs the shared round schedule or the shared pool verifier (product_schedule.hpp), for a per-launch
view, at two batches: 16 x 2^20, and a mixed one of 2^11, 2^12 and 2^13 (2^11: round 0, then one bind pass whose sums nobody reads).
The entries, in this order per batch: product (d = 3), sop (pool of 3; a b - c), zero-check (the same pool and terms), verify sop,
verify zero-check.  The tables are uploaded first, in three copies.

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o t -- python3 tools/trace_product_family.py
    python3 tools/trace_product_family.py --summarize DIR      (kernel names with their launch counts; copies by direction)

A run of its own: no counters.  Two builds launch the same when their summaries are equal line for line."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = [("16x2^20", [20] * 16), ("mixed 2^11..2^13", [11, 12, 13, 13, 12, 11])]
P = 2013265921


def run():
    import numpy as np
    import zigz_amd
    import oracle_lib as O
    ctx = zigz_amd.Context(0)
    n_max = 1 << 20
    tabs = []
    for j in range(3):
        tabs.append(ctx.dev_alloc(4 * n_max))
        ctx.upload(O.splitmix64_field(7 + j, n_max), tabs[-1])  # (a shorter instance reads a prefix)
    terms = [(1, (0, 1)), (P - 1, (2,))]
    for name, vs in BATCHES:
        ns = [1 << v for v in vs]
        taus = [[int(x) for x in O.splitmix64_field(100 + i, v)] for i, v in enumerate(vs)]
        ctx.dev_sumcheck_prove_product_batch([tabs] * len(ns), ns)
        sop = ctx.dev_sumcheck_prove_sop_batch([(tabs, terms)] * len(ns), ns)
        zc = ctx.dev_sumcheck_prove_zerocheck_batch([(tabs, terms, tau) for tau in taus], ns)
        rej = ctx.dev_sumcheck_verify_sop_batch([(tabs, terms)] * len(ns), ns, sop, 1)[3]
        rej += ctx.dev_sumcheck_verify_zerocheck_batch([(tabs, terms, tau) for tau in taus], ns, zc, 1)[3]
        assert rej == 0, name
    ctx.close()


def summarize(d):
    def rows(pattern):
        return [r for f in sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True)) for r in csv.DictReader(open(f))]
    kernels, copies = {}, {}
    for r in rows("*kernel_trace.csv"):
        k = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("zk::", "")
        kernels[k] = kernels.get(k, 0) + 1
    for r in rows("*memory_copy_trace.csv"):
        copies[r["Direction"]] = copies.get(r["Direction"], 0) + 1
    print("kernel,launches")
    for k in sorted(kernels):
        print(f"{k},{kernels[k]}")
    print("copy,count")
    for k in sorted(copies):
        print(f"{k},{copies[k]}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run()
