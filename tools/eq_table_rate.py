#!/usr/bin/env python3
"""Batched eq tables and batched product-proof verification on one MI355X, in one process (warm-up first, then the forms
alternate rep by rep; medians of --reps with the spread), at 1024 x 2^10, 256 x 2^14, 16 x 2^20 and 1 x 2^24:

  eq      zigz_dev_eq_table_batch (one copy, one launch; timed until the stream has drained) against the only route there was
          before it: zigz_dev_upload_u64 of host-built tables of the same sizes -- ONE upload call of all of them, the upload
          alone, not the host's build.  The device form's end-to-end TB/s of 4 N written bytes.
  verify  zigz_dev_sumcheck_verify_product_batch (POINT_REVERSED, all accepting) over proofs of the product prover at d = 1, 2, 3
          with table factors, at d = 3 with eq(tau, .) as the first factor (given by tau alone), and at d = 1 against
          zigz_dev_sumcheck_verify_batch over the same proofs; the host's share alone (replay and eq factors) from the stand-alone
          driver tests/c_driver/product_verify_host.cpp, built here with g++ -O2.

    python tools/eq_table_rate.py [--reps R] [--quick]      (prints one JSON object)
    python tools/eq_table_rate.py --kernel-times DB         (prints one JSON object)
    python tools/eq_table_rate.py --raw-d1 [--reps R]       (prints one JSON object)

--quick: two reps of each form, for a kernel trace (rocprofv3 --kernel-trace --stats in a run of its own).  --kernel-times reads
that run's database: the kernel times of k_eq_batch_expand and k_mle_batch_eval per shape (the launches are told apart by their
order and workgroup counts), k_eq_batch_expand's against 4 B per word at the 8 TB/s the README prices k_radix_fold with.  The end-to-end
times go through the ctypes faces, which concatenate the proofs per call: at the small shapes they measure that marshalling as
much as the library; --raw-d1 times the two verify entries at d = 1 through ctypes calls whose arrays are marshalled once, outside
the timed region.
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

SHAPES = [("1024x2^10", 1024, 10), ("256x2^14", 256, 14), ("16x2^20", 16, 20), ("1x2^24", 1, 24)]
BAR = ("16x2^20", "1x2^24")  # where the device form must not lose to the upload: its max below the upload's min


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(xs.min()), 4), "max_ms": round(float(xs.max()), 4)}


def alternate(forms, reps):
    """forms: {name: callable}; two warm-ups, then the forms alternate rep by rep"""
    acc = {name: [] for name in forms}
    for _ in range(2):
        for f in forms.values():
            f()
    for _ in range(reps):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            acc[name].append(time.perf_counter() - t0)
    return {name: stats(ts) for name, ts in acc.items()}


def kernel_times(db):
    """kernel times per shape from a rocprofv3 --kernel-trace database of one --quick run.  Two shapes can have the same
    workgroup count (16 x 2^20 and 1 x 2^24 are 2048 chunks each), so the launches are first cut into the tool's shapes by
    their order: a shape's section begins with its first k_eq_batch_expand launch, which follows the last k_mle_batch_eval
    launch of the shape before."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, grid_x, end - start from kernels where name like '%k_eq_batch_expand%' "
                                       "or name like '%k_mle_batch_eval%' order by start").fetchall()
    sections, last_eq = [], False
    for name, grid, dur in rows:
        is_eq = "k_eq_batch_expand" in name
        if is_eq and not last_eq:
            sections.append([])
        last_eq = is_eq
        sections[-1].append(("k_eq_batch_expand" if is_eq else "k_mle_batch_eval", grid // 256, dur / 1e3))
    assert len(sections) == len(SHAPES), len(sections)
    out = {"k_eq_batch_expand": {}, "k_mle_batch_eval": {}}
    for (name, k, v), sec in zip(SHAPES, sections):
        chunks = k * (((1 << v) + 8191) // 8192)
        for kern, factors in (("k_eq_batch_expand", 1), ("k_mle_batch_eval", 1), ("k_mle_batch_eval", 2), ("k_mle_batch_eval", 3)):
            us = sorted(d for kn, g, d in sec if kn == kern and g == chunks * factors)
            if not us:
                continue
            n, med = factors * k << v, us[len(us) // 2]
            out[kern][name if kern == "k_eq_batch_expand" else f"{name}, {factors} table factor(s) per proof"] = {
                "launches": len(us), "median_us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                "hbm_bound_us_4N_at_8TBps": round(4 * n / 8e12 * 1e6, 2), "TBps_4N": round(4 * n / med / 1e6, 3)}
    return out


def build_driver(tmp):
    csrc = os.path.join(ROOT, "zigz_amd", "csrc")
    exe = os.path.join(tmp, "product_verify_host")
    srcs = [os.path.join(csrc, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "c_driver", "product_verify_host.cpp")] + srcs + ["-o", exe])
    return exe


def replay_alone(exe, tmp, proofs, taus, reps):
    """the driver's `time` over the proofs; taus[i]: the tau of proof i's eq first factor, or None"""
    path = os.path.join(tmp, "proofs.txt")
    with open(path, "w") as fh:
        for (c, r, q, ev, fe), tau in zip(proofs, taus):
            d = len(ev)
            words = [d, len(q), 1, 1, c, fe, *r, *q, *ev]
            for j in range(d):
                words += [1, *tau] if (j == 0 and tau is not None) else [0, ev[j]]
            fh.write(" ".join(str(int(x)) for x in words) + "\n")
    w = subprocess.run([exe, "time", path, str(reps)], capture_output=True, text=True, check=True).stdout.split()
    assert w[0] == "replay_ms" and int(w[4]) == len(proofs), w
    return {"median_ms": round(float(w[1]), 4), "min_ms": round(float(w[2]), 4), "max_ms": round(float(w[3]), 4)}


def raw_d1(reps):
    """d = 1 proofs verified by both entries through ctypes calls whose arrays are marshalled ONCE, outside the timed region:
    what the product entry itself costs against the linear one, without the Python faces"""
    import ctypes as C

    import zigz_amd
    from zigz_amd import hip
    from zigz_amd._ffi import lib, u8p, u64p, vp

    ctx = zigz_amd.Context(0)
    rng = np.random.default_rng(13)
    out = {"reps": reps, "shapes": {}}
    for name, k, v in SHAPES:
        n = 1 << v
        base = ctx.dev_alloc(4 * k * n)
        ctx.upload(rng.integers(0, hip.P, size=k * n, dtype=np.uint64), base)
        ptrs = [base + 4 * n * i for i in range(k)]
        proofs = ctx.dev_sumcheck_prove_product_batch([[p] for p in ptrs], [n] * k)
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in xs]))
        cs, rr, qq, ff = cat([[p[0]] for p in proofs]), cat([p[1] for p in proofs]), cat([p[2] for p in proofs]), cat([[p[4]] for p in proofs])
        pa, ns, dg = (vp * k)(*ptrs), (C.c_size_t * k)(*[n] * k), (C.c_uint * k)(*[1] * k)
        verd, exp, orc = np.zeros(k, dtype=np.uint8), np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        u = lambda a: a.ctypes.data_as(u64p)

        def product():
            rc = lib.zigz_dev_sumcheck_verify_product_batch(ctx.h, k, dg, pa, None, None, ns, u(cs), u(rr), u(qq), None, u(ff), 1,
                                                            verd.ctypes.data_as(u8p), u(exp), u(orc), C.byref(rej), C.byref(bad))
            assert rc == 0 and rej.value == 0

        def linear():
            rc = lib.zigz_dev_sumcheck_verify_batch(ctx.h, pa, ns, k, u(cs), u(rr), u(qq), u(ff), 1, verd.ctypes.data_as(u8p), u(exp),
                                                    u(orc), C.byref(rej), C.byref(bad))
            assert rc == 0 and rej.value == 0

        out["shapes"][name] = alternate({"product_entry_d1": product, "linear_entry": linear}, reps)
        ctx.dev_free(base)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps of each form (for a kernel trace)")
    ap.add_argument("--kernel-times", metavar="DB", help="read the kernel times from a rocprofv3 database")
    ap.add_argument("--raw-d1", action="store_true", help="d = 1: both verify entries through pre-marshalled ctypes calls only")
    a = ap.parse_args()
    if a.raw_d1:
        print(json.dumps(raw_d1(a.reps)))
        return
    if a.kernel_times:
        print(json.dumps(kernel_times(a.kernel_times)))
        return
    tmp = tempfile.mkdtemp()
    driver = None if a.quick else build_driver(tmp)
    reps = 2 if a.quick else a.reps
    import zigz_amd
    from zigz_amd import hip

    P = hip.P
    REV = hip.SUMCHECK_VERIFY_POINT_REVERSED
    ctx = zigz_amd.Context(0)
    out = {"reps": reps, "launches_per_call": {"eq_table_batch": 1, "verify_product_batch": 2, "copies": 1}, "shapes": {}}
    rng = np.random.default_rng(11)
    for name, k, v in SHAPES:
        n = 1 << v
        ns = [n] * k
        words = k * n
        base = ctx.dev_alloc(4 * words * 4)  # eq tables | three factor tables per instance
        eq_ptrs = [base + 4 * n * i for i in range(k)]
        tab_ptrs = [[base + 4 * (words * (1 + j) + n * i) for j in range(3)] for i in range(k)]
        taus = [rng.integers(0, P, size=v, dtype=np.uint64) for _ in range(k)]
        host_tables = rng.integers(0, P, size=words, dtype=np.uint64)  # what the caller would have built on the host

        def eq():
            ctx.dev_eq_table_batch(eq_ptrs, ns, taus)
            ctx.synchronize()

        def upload():
            ctx.upload(host_tables, base)

        res = {"words": words}
        t = alternate({"upload_u64": upload, "dev_eq_table_batch": eq}, reps)
        eq()
        first = ctx.download(eq_ptrs[0], n)
        res["eq_sums_to_one"] = int(first.sum(dtype=np.uint64)) % P == 1
        res.update(t)
        res["eq_TBps_4N"] = round(4 * words / (t["dev_eq_table_batch"]["median_ms"] * 1e-3) / 1e12, 4)
        res["eq_fraction_of_8TBps"] = round(res["eq_TBps_4N"] / 8, 4)
        res["eq_max_below_upload_min"] = t["dev_eq_table_batch"]["max_ms"] < t["upload_u64"]["min_ms"]
        if name in BAR:
            assert res["eq_max_below_upload_min"], (name, t)
        # verification: d = 1, 2, 3 over table factors, d = 3 with the eq table as the first factor
        for j in range(3):
            ctx.upload(rng.integers(0, P, size=words, dtype=np.uint64), base + 4 * words * (1 + j))
        forms, proofs_of = {}, {}
        for d in (1, 2, 3):
            inst = [tp[:d] for tp in tab_ptrs]
            proofs = ctx.dev_sumcheck_prove_product_batch(inst, ns)
            proofs_of[f"d{d}"] = (proofs, [None] * k)
            forms[f"verify_d{d}"] = (lambda inst=inst, proofs=proofs: ctx.dev_sumcheck_verify_product_batch(inst, ns, proofs, REV))
        inst_eq = [[e] + tp[:2] for e, tp in zip(eq_ptrs, tab_ptrs)]
        proofs_eq = ctx.dev_sumcheck_prove_product_batch(inst_eq, ns)
        proofs_of["d3_eq"] = (proofs_eq, taus)
        inst_tau = [[None] + tp[:2] for tp in tab_ptrs]
        forms["verify_d3_eq_first"] = lambda: ctx.dev_sumcheck_verify_product_batch(inst_tau, ns, proofs_eq, REV, taus=taus)
        p1 = proofs_of["d1"][0]
        lin = [(p[1], p[2], p[4]) for p in p1]
        forms["linear_verify_d1"] = lambda: ctx.dev_sumcheck_verify_batch([tp[0] for tp in tab_ptrs], ns, [p[0] for p in p1], lin, REV)
        res["all_accept"] = all(int(f()[3]) == 0 for f in forms.values())
        res.update(alternate(forms, reps))
        if driver:
            res["host_replay_alone"] = {key: replay_alone(driver, tmp, pr, ts, reps) for key, (pr, ts) in proofs_of.items()}
        out["shapes"][name] = res
        ctx.dev_free(base)
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
