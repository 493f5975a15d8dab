#!/usr/bin/env python3
"""Many openings per committed tree on one MI355X, in one process (warm-up first, then the forms alternate rep by rep):

  shapes   43 x 20, 4096 x 20, 2^16 x 20 and 2^20 x 20 openings of one 2^20-value table, and 2^16 openings spread over 23
           tables of 2^0 .. 2^22 values
  loop     the baseline: k calls of zigz_merkle_open on a zigz_merkle of the same values (all k at the two small shapes,
           4096 calls at the larger ones: per-opening time)
  hform    zigz_merkle_open_many into host arrays, against one pinned device-to-host copy of the same output bytes
  dform    zigz_dev_merkle_open_many into device arrays (call + stream wait), against a device-to-device copy of the same
           output bytes measured in the same run
  cross    one open_many call vs the loop for k = 1 .. 4096: the k from which one call is faster

Every shape's host-form output is checked against the loop's openings (a sample) and through zigz_merkle_verify_batch.

    python tools/merkle_open_many_rate.py [--reps R] [--quick] [--out profiles/merkle_open_many_rate.json]
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


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps, no crossover (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = 2 if a.quick else a.reps
    import torch
    import zigz_amd
    import oracle_lib as O

    ctx = zigz_amd.Context(0)
    big = O.splitmix64_field(1, 1 << 20)
    res20, b20 = ctx.merkle_commit_batch([big])
    single = zigz_amd.SimpleMerkleTree(ctx, big)
    assert single.root_hash == res20[0][0]
    mix_tables = [O.splitmix64_field(100 + v, 1 << v) for v in range(23)]
    _, bmix = ctx.merkle_commit_batch(mix_tables)

    def timed(fns, reps):
        for fn in fns.values():
            fn()  # warm-up
        t = {f: [] for f in fns}
        for _ in range(reps):
            for f, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                t[f].append(time.perf_counter() - t0)
        return {f: median(v) for f, v in t.items()}

    def d2d(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def run():
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
        return run

    def d2h(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

        def run():
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
        return run

    def loop(indices):
        def run():
            return [single.open(int(i)) for i in indices]
        return run

    def dform(b, trees, indices, tot):
        k = len(trees)
        bufs = [torch.empty(32 * tot + 32, dtype=torch.uint8, device="cuda"), torch.empty(tot + 32, dtype=torch.uint8, device="cuda"),
                torch.empty(k + 1, dtype=torch.int64, device="cuda"), torch.empty(32 * k + 32, dtype=torch.uint8, device="cuda")]
        torch.cuda.synchronize()

        def run():
            b.dev_open_many(trees, indices, *[x.data_ptr() for x in bufs])
            ctx.synchronize()
        return run

    rng = np.random.default_rng(5)
    out = {"reps": reps}
    shapes = [("43x20", b20, 43), ("4096x20", b20, 4096), ("2^16x20", b20, 1 << 16), ("2^20x20", b20, 1 << 20), ("mix_2^0..2^22_x2^16", bmix, 1 << 16)]
    for name, b, k in shapes:
        if b is b20:
            trees = np.zeros(k, dtype=np.uint32)
            indices = rng.integers(0, 1 << 20, size=k).astype(np.uint64)
        else:
            trees = rng.integers(0, 23, size=k).astype(np.uint32)
            indices = (rng.integers(0, 1 << 62, size=k).astype(np.uint64) % (np.uint64(1) << trees.astype(np.uint64)))
        tot = int(np.asarray(b.heights)[trees].sum())
        nbytes = 33 * tot + 40 * k
        got = b.open_many(trees, indices)
        verd = ctx.merkle_verify_batch(got["roots"], got["heights"], got["leaves"], got["siblings"], got["dirs"])
        assert int((verd == 0).sum()) == 0
        n_loop = min(k, 4096)
        if b is b20:
            for j, o in zip(range(64), loop(indices[:64])()):
                assert got["siblings"][640 * j: 640 * (j + 1)].tobytes() == o["siblings"] and int(got["leaves"][j]) == o["value"]
        fns = {"hform": lambda: b.open_many(trees, indices), "d2h_copy": d2h(nbytes), "dform": dform(b, trees, indices, tot),
               "d2d_copy": d2d(nbytes)}
        t = timed(fns, reps)
        r = dict(k=k, sibling_slots=tot, out_bytes=nbytes, ms={f: round(v * 1e3, 4) for f, v in t.items()})
        if b is b20:
            tl = timed({"loop": loop(indices[:n_loop])}, reps if n_loop <= 43 else min(reps, 3))["loop"]
            per = tl / n_loop
            r["loop_calls"] = n_loop
            r["ms"]["loop"] = round(tl * 1e3, 4)
            r["loop_us_per_opening"] = round(per * 1e6, 3)
            r["hform_speedup_over_loop"] = round(per * k / t["hform"], 1)
            r["dform_speedup_over_loop"] = round(per * k / t["dform"], 1)
        r["hform_us_per_opening"] = round(t["hform"] / k * 1e6, 4)
        r["dform_us_per_opening"] = round(t["dform"] / k * 1e6, 4)
        r["dform_over_d2d_copy"] = round(t["dform"] / t["d2d_copy"], 2)
        r["hform_over_d2h_copy"] = round(t["hform"] / t["d2h_copy"], 2)
        r["dform_out_GB_per_s"] = round(nbytes / t["dform"] / 1e9, 2)
        r["d2d_copy_GB_per_s"] = round(nbytes / t["d2d_copy"] / 1e9, 2)
        out[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    if not a.quick:
        cross = {}
        for k in (1, 2, 4, 8, 16, 43, 64, 256, 1024, 4096):
            trees = np.zeros(k, dtype=np.uint32)
            indices = rng.integers(0, 1 << 20, size=k).astype(np.uint64)
            t = timed({"loop": loop(indices), "hform": lambda: b20.open_many(trees, indices), "dform": dform(b20, trees, indices, 20 * k)},
                      reps if k <= 256 else min(reps, 3))
            cross[k] = {f: round(v * 1e6, 1) for f, v in t.items()}
            print("cross", k, cross[k], file=sys.stderr, flush=True)
        out["crossover_us_height20"] = cross
        out["crossover_k_one_call_faster_from"] = {
            f: next((k for k in sorted(cross) if cross[k][f] < cross[k]["loop"]), None) for f in ("hform", "dform")}
    single.deinit()
    b20.deinit()
    bmix.deinit()
    s = json.dumps(out)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
