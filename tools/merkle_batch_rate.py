#!/usr/bin/env python3
"""Batched vs single Merkle commitments on one MI355X, in one process (warm-up first, then the forms alternate rep by rep):

  shapes   1024 x 2^10, 256 x 2^14, 16 x 2^20 and one mixed batch of 2^0 ... 2^22
  batch    zigz_merkle_commit_batch + zigz_commit_open_batch (host tables, end to end), the commit alone, and
           zigz_dev_merkle_commit_batch alone over device-resident tables (no upload)
  single   k x (zigz_merkle_commit + zigz_commit_open over the stored values + zigz_merkle_destroy)

Permutations: a tree of npad leaves is 2 npad - 1 Keccak-f permutations; the rates are set against the ~13 G/s of the dense leaf
kernel.  Every batch root is compared with its single call's.

    python tools/merkle_batch_rate.py [--reps R] [--quick]      (prints one JSON object)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CEILING = 13e9  # permutations / s of k_keccak_leaves


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form (for a kernel trace)")
    a = ap.parse_args()
    reps = 2 if a.quick else a.reps
    import zigz_amd
    import oracle_lib as O

    P = O.P_BB
    ctx = zigz_amd.Context(0)
    shapes = [("1024x2^10", [1 << 10] * 1024), ("256x2^14", [1 << 14] * 256), ("16x2^20", [1 << 20] * 16),
              ("mixed_2^0..2^22", [1 << v for v in range(23)])]
    out = {"reps": reps, "ceiling_perms_per_s": CEILING}
    for name, ns in shapes:
        tables = [O.splitmix64_field(17 + i, n) for i, n in enumerate(ns)]
        rng = np.random.default_rng(1)
        points = [[int(x) for x in rng.integers(0, P, size=n.bit_length() - 1)] for n in ns]
        perms = sum(2 * n - 1 for n in ns)
        # device-resident copies for the dev form (one buffer, 16-byte aligned tables)
        off, o = [], 0
        for n in ns:
            off.append(o)
            o += (n + 3) // 4 * 4
        packed = np.zeros(o, dtype=np.uint64)
        for t, x in zip(tables, off):
            packed[x:x + len(t)] = t
        d_base = ctx.dev_alloc(o * 4)
        ctx.upload(packed, d_base)
        d_ptrs = [d_base + 4 * x for x in off]

        def batch_full():
            res, b = ctx.merkle_commit_batch(tables)
            op = ctx.commit_open_batch(b, points)
            b.deinit()
            return res, op

        def batch_commit():
            return ctx.merkle_commit_batch(tables, keep=False)[0]

        def dev_commit():
            return ctx.dev_merkle_commit_batch(d_ptrs, ns, keep=False)[0]

        def singles():
            res, op = [], []
            for t, pt in zip(tables, points):
                s = zigz_amd.SimpleMerkleTree(ctx, t)
                op.append(zigz_amd.CommitmentScheme.open(ctx, None, s, pt))
                res.append((s.root_hash, s.height))
                s.deinit()
            return res, op

        forms = {"batch_commit_open": batch_full, "batch_commit": batch_commit, "dev_batch_commit": dev_commit,
                 "single_commit_open": singles}
        first = {f: fn() for f, fn in forms.items()}  # warm-up (and the results compared below)
        times = {f: [] for f in forms}
        for _ in range(reps):
            for f, fn in forms.items():
                t0 = time.perf_counter()
                fn()
                times[f].append(time.perf_counter() - t0)
        ctx.dev_free(d_base)
        sres, sop = first["single_commit_open"]
        bres, bop = first["batch_commit_open"]
        ms = {f: round(median(v) * 1e3, 3) for f, v in times.items()}
        r = dict(k=len(ns), perms=perms, ms=ms,
                 parity=bres == sres and first["batch_commit"] == sres and first["dev_batch_commit"] == sres and bop == sop,
                 speedup_commit_open=round(ms["single_commit_open"] / ms["batch_commit_open"], 2))
        for f in ("batch_commit", "dev_batch_commit", "batch_commit_open", "single_commit_open"):
            rate = perms / (ms[f] * 1e-3)
            r[f + "_Gperms_per_s"] = round(rate / 1e9, 3)
            r[f + "_of_ceiling"] = round(rate / CEILING, 3)
        out[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
