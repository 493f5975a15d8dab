#!/usr/bin/env python3
"""Batched MLE evaluation and batched sumcheck verification on one MI355X, in one process (warm-up first, then the forms alternate
rep by rep; medians of --reps with the spread):

  eval    zigz_dev_mle_eval_batch over device-resident tables against a loop of zigz_dev_mle_eval calls over the same tables and
          points, at the shapes of DESIGN.md s7b: 1024 x 2^10, 256 x 2^14, 16 x 2^20 and the 23 tables 2^0 .. 2^22; the
          batch's end-to-end TB/s of 4 N algorithmic bytes (N = all elements)
  verify  zigz_dev_sumcheck_verify_batch (POINT_REVERSED) over proofs of the same tables from the batched prover, against the
          host's replay of the same proofs alone -- the stand-alone driver tests/c_driver/sumcheck_verify_host.cpp, built here
          with g++ -O2, runs sv::replay_rounds on the library's host threads and nothing else -- and against the batched
          evaluation of the final points alone: whether the evaluation hides under the replay

    python tools/mle_eval_batch_rate.py [--reps R] [--quick]      (prints one JSON object)
    python tools/mle_eval_batch_rate.py --kernel-times DB         (prints one JSON object)

--quick: two reps of each form, for a kernel trace (rocprofv3 --kernel-trace --stats in a run of its own).  --kernel-times reads
that run's database: the kernel time of k_mle_batch_eval per shape (the launches are told apart by their workgroup counts)
against 4 B per element at the 8 TB/s the README prices k_radix_fold with.  The end-to-end times go through the ctypes face,
which concatenates the k points per call: at the small shapes they measure that marshalling as much as the library.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1024x2^10", [10] * 1024), ("256x2^14", [14] * 256), ("16x2^20", [20] * 16), ("2^0..2^22", list(range(23)))]


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(xs.min()), 4), "max_ms": round(float(xs.max()), 4)}


def workgroups(logs):
    return sum(((1 << v) + 8191) // 8192 for v in logs)


def kernel_times(db):
    """k_mle_batch_eval's kernel time per shape from a rocprofv3 --kernel-trace database"""
    import sqlite3
    rows = sqlite3.connect(db).execute("select grid_x, end - start from kernels where name like '%k_mle_batch_eval%'").fetchall()
    out = {}
    for name, logs in SHAPES:
        us = sorted(d / 1e3 for g, d in rows if g // 256 == workgroups(logs))
        if us:
            n = sum(1 << v for v in logs)
            med = us[len(us) // 2]
            out[name] = {"launches": len(us), "median_us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                         "hbm_bound_us_4N_at_8TBps": round(4 * n / 8e12 * 1e6, 2), "TBps_4N": round(4 * n / med / 1e6, 3)}
    return out


def build_driver(tmp):
    csrc = os.path.join(ROOT, "zigz_amd", "csrc")
    exe = os.path.join(tmp, "sumcheck_verify_host")
    srcs = [os.path.join(csrc, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "c_driver", "sumcheck_verify_host.cpp")] + srcs + ["-o", exe])
    return exe


def replay_alone(exe, tmp, sums, proofs, reps):
    path = os.path.join(tmp, "proofs.txt")
    with open(path, "w") as fh:
        for c, (r, q, f) in zip(sums, proofs):
            fh.write(" ".join(str(int(x)) for x in [len(q), c, f, *r, *q]) + "\n")
    w = subprocess.run([exe, "time", path, str(reps)], capture_output=True, text=True, check=True).stdout.split()
    assert w[0] == "replay_ms" and int(w[4]) == len(proofs), w
    return {"median_ms": round(float(w[1]), 4), "min_ms": round(float(w[2]), 4), "max_ms": round(float(w[3]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form (for a kernel trace)")
    ap.add_argument("--kernel-times", metavar="DB", help="read k_mle_batch_eval's kernel times from a rocprofv3 database")
    a = ap.parse_args()
    if a.kernel_times:
        print(json.dumps({"k_mle_batch_eval": kernel_times(a.kernel_times)}))
        return
    tmp = tempfile.mkdtemp()
    driver = None if a.quick else build_driver(tmp)
    reps = 2 if a.quick else a.reps
    import zigz_amd
    from zigz_amd import hip

    P = hip.P
    ctx = zigz_amd.Context(0)
    out = {"reps": reps, "launches_per_call": {"eval_batch": 2, "copies": 1}, "shapes": {}}
    rng = np.random.default_rng(7)
    for name, logs in SHAPES:
        ns = [1 << v for v in logs]
        offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in ns])]).astype(np.int64)
        packed = rng.integers(0, P, size=int(offs[-1]), dtype=np.uint64)
        base = ctx.dev_alloc(len(packed) * 4)
        ctx.upload(packed, base)
        ptrs = [base + 4 * int(o) for o in offs[:-1]]
        pts = [rng.integers(0, P, size=v, dtype=np.uint64) for v in logs]

        def batch():
            return ctx.dev_mle_eval_batch(ptrs, ns, pts)

        def loop():
            return [ctx.dev_mle_eval(p, n, q) for p, n, q in zip(ptrs, ns, pts)]

        res = {"parity": batch() == loop(), "elements": int(sum(ns))}
        tb, tl = [], []
        for _ in range(2):
            batch(), loop()
        for _ in range(reps):
            for form, acc in ((batch, tb), (loop, tl)):
                t0 = time.perf_counter()
                form()
                acc.append(time.perf_counter() - t0)
        res["batch"], res["loop"] = stats(tb), stats(tl)
        res["speedup"] = round(res["loop"]["median_ms"] / res["batch"]["median_ms"], 2)
        res["batch_TBps_4N"] = round(4 * sum(ns) / (res["batch"]["median_ms"] * 1e-3) / 1e12, 4)
        # verification of the same tables' proofs (tables of one value have no proof)
        sel = [i for i, n in enumerate(ns) if n > 1]
        vptrs, vns = [ptrs[i] for i in sel], [ns[i] for i in sel]
        proofs = ctx.dev_sumcheck_prove_batch(vptrs, vns)
        sums = [int(packed[int(offs[i]):int(offs[i]) + ns[i]].sum() % P) for i in sel]
        rev = [np.asarray(p[1])[::-1].copy() for p in proofs]

        def verify():
            return ctx.dev_sumcheck_verify_batch(vptrs, vns, sums, proofs, hip.SUMCHECK_VERIFY_POINT_REVERSED)

        def eval_only():
            return ctx.dev_mle_eval_batch(vptrs, vns, rev)

        verd, _, orc, rej = verify()
        res["verify_all_accept"] = bool(rej == 0 and verd.all()) and orc == eval_only()
        tv, te = [], []
        for _ in range(2):
            verify(), eval_only()
        for _ in range(reps):
            for form, acc in ((verify, tv), (eval_only, te)):
                t0 = time.perf_counter()
                form()
                acc.append(time.perf_counter() - t0)
        res["verify"], res["eval_of_the_final_points"] = stats(tv), stats(te)
        if driver:
            res["host_replay_alone"] = replay_alone(driver, tmp, sums, proofs, reps)
        out["shapes"][name] = res
        ctx.dev_free(base)
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
