#!/usr/bin/env python3
"""Batched vs sequential provers on one MI355X, in one process (warm-up first, then the two forms alternate rep by rep):

  sumcheck  16 device-resident tables of 2^20: zigz_dev_sumcheck_prove_batch against 16 zigz_dev_sumcheck_prove calls, warm and
            cold (a 1 GiB read sweep before every rep: 16 x 2^20 x 4 B = 64 MiB would otherwise sit in the 256 MiB Infinity
            Cache, which flatters the fold's second read); end-to-end TB/s of 12 N algorithmic bytes (N = all elements)
  lasso     16 instances of 2^16 queries over 2^16-row tables: zigz_lasso_prove_batch against 16 zigz_lasso_prove calls, and
            the host-sponge share: the 2k flat commitments alone, run as 2k sequential SHA3 sponges over the same bytes

    python tools/sumcheck_batch_rate.py [--reps R] [--quick]      (prints one JSON object)
"""
import argparse
import hashlib
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="a few reps of each form (for a kernel trace)")
    a = ap.parse_args()
    reps = 3 if a.quick else a.reps
    import torch
    import zigz_amd
    import oracle_lib as O

    P = O.P_BB
    ctx = zigz_amd.Context(0)
    out = {"reps": reps}
    k, nv = 16, 20
    n = 1 << nv
    rng = np.random.default_rng(20)
    tabs = rng.integers(0, P, size=(k, n), dtype=np.uint64)
    base = ctx.dev_alloc(k * n * 4)
    ctx.upload(tabs.reshape(-1), base)
    ptrs = [base + i * n * 4 for i in range(k)]
    flush = torch.empty(1 << 28, dtype=torch.int32, device="cuda")  # 1 GiB, read-only sweep
    flush.fill_(1)
    torch.cuda.synchronize()

    def batch():
        return ctx.dev_sumcheck_prove_batch(ptrs, [n] * k)

    def seq():
        return [ctx.dev_sumcheck_prove(p, n) for p in ptrs]

    # parity first: the batch is the sequential calls' bytes
    b, s = batch(), seq()
    out["sumcheck_parity"] = all(O.sumcheck_to_bytes(*x) == O.sumcheck_to_bytes(*y) for x, y in zip(b, s))
    for cold in (False, True):
        tb, ts = [], []
        for _ in range(3):
            batch(), seq()
        for _ in range(reps):
            for form, acc in ((batch, tb), (seq, ts)):
                if cold:
                    torch.cuda.synchronize()
                    flush.sum()
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                form()
                acc.append(time.perf_counter() - t0)
        tag = "cold" if cold else "warm"
        bms, sms = median(tb) * 1e3, median(ts) * 1e3
        out[f"sumcheck_16x2^20_{tag}"] = {
            "batch_ms": round(bms, 4), "sequential_ms": round(sms, 4), "speedup": round(sms / bms, 2),
            "batch_TBps_12N": round(12 * k * n / (bms * 1e-3) / 1e12, 3),
            "sequential_TBps_12N": round(12 * k * n / (sms * 1e-3) / 1e12, 3)}
    ctx.dev_free(base)
    del flush

    # Lasso: 16 x (2^16 queries over a 2^16-row table)
    bits, nq, kl = 8, 1 << 16, 16
    insts = []
    for i in range(kl):
        tab = np.asarray(O.build_table(P, i % 3, bits), dtype=np.uint64)
        q = tab[rng.integers(0, len(tab), size=nq)]
        insts.append(dict(table=tab, queries=q))
    lb = ctx.lasso_prove_batch(insts)
    ls = [ctx.lasso_prove(d["table"], d["queries"]) for d in insts]
    out["lasso_parity"] = all(x["query_commit"] == y["query_commit"] and x["table_commit"] == y["table_commit"] and
                              x["final_eval"] == y["final_eval"] and np.array_equal(x["rounds"], y["rounds"]) for x, y in zip(lb, ls))
    tb, ts = [], []
    for _ in range(reps):
        for form, acc in ((lambda: ctx.lasso_prove_batch(insts), tb),
                          (lambda: [ctx.lasso_prove(d["table"], d["queries"]) for d in insts], ts)):
            t0 = time.perf_counter()
            form()
            acc.append(time.perf_counter() - t0)
    # host-sponge share: the 2k flat commitments alone (sequential sponges over the same LE64 fingerprint bytes)
    fps = []
    for d in insts:
        fps.append(np.asarray(ctx.lasso_fingerprints(d["table"]), dtype=np.uint64).tobytes())
        qf = np.zeros(nq, dtype=np.uint64)
        qf[:] = ctx.lasso_fingerprints(d["queries"])
        fps.append(qf.tobytes())
    t0 = time.perf_counter()
    for f in fps:
        hashlib.sha3_256(f).digest()
    sponge_ms = (time.perf_counter() - t0) * 1e3
    bms, sms = median(tb) * 1e3, median(ts) * 1e3
    out["lasso_16x2^16"] = {"batch_ms": round(bms, 3), "sequential_ms": round(sms, 3), "speedup": round(sms / bms, 2),
                            "sequential_sponges_ms_all_2k": round(sponge_ms, 3)}
    out["host_keccak"] = zigz_amd._ffi.lib.zigz_host_keccak_impl().decode()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
