#!/usr/bin/env python3
"""Batched Merkle verification on one MI355X, in one process (warm-up first, then the forms alternate rep by rep):

  shapes   43 x 20 (one proof's openings), 4096 x 20, 2^16 x 20, 2^20 x 20 and a mix of heights 0 .. 24
  host     CommitmentScheme::batchVerify of the C++ host (zigzh_batch_verify): one thread, one SHA3 call per permutation
  hform    zigz_merkle_verify_batch from host arrays (staging, upload, verify), against the time of one pinned host-to-device
           copy of the same bytes measured in the same run
  dform    zigz_dev_merkle_verify_batch over device-resident openings, in G permutations/s against the ~13 G/s of the dense
           leaf kernel; A/B of the hash with and without the re-arm pauses (option "verify_pause")
  cross    host vs both forms for k = 1 .. 4096 openings of height 20: the k below which the host is faster

An opening of height h is h + 1 Keccak-f permutations.  The openings are honest paths of a few committed tables (opened on the
device), about 1 % tampered, tiled to the shape's k; every form's verdicts are compared with the host's.

    python tools/merkle_verify_rate.py [--reps R] [--quick] [--out profiles/merkle_verify_rate.json]
"""
import argparse
import ctypes as C
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


class Openings:
    """k openings as the C arrays (roots, heights, leaves, siblings, dirs), on the host and on the device"""

    def __init__(self, roots, heights, leaves, sib, dirs):
        import torch
        self.k = len(heights)
        self.roots = np.ascontiguousarray(roots, dtype=np.uint8)
        self.heights = (C.c_size_t * self.k)(*[int(h) for h in heights])
        self.hlist = [int(h) for h in heights]
        self.leaves = np.ascontiguousarray(leaves, dtype=np.uint64)
        self.sib = np.ascontiguousarray(sib, dtype=np.uint8)
        self.dirs = np.ascontiguousarray(dirs, dtype=np.uint8)
        self.perms = int(sum(self.hlist)) + self.k
        self.bytes = self.roots.nbytes + self.leaves.nbytes + self.sib.nbytes + self.dirs.nbytes
        self.d = [torch.from_numpy(a).to("cuda") for a in (self.roots, self.leaves, self.sib, self.dirs)]
        torch.cuda.synchronize()


def make_pool(ctx, P, heights, seed):
    """honest openings, one per entry of `heights` (each a table of 2^h values committed once), about 1 % tampered"""
    import oracle_lib as O
    uniq = sorted(set(heights))
    tables = {h: O.splitmix64_field(seed + h, 1 << h) for h in uniq}
    res, b = ctx.merkle_commit_batch([tables[h] for h in heights])
    rng = np.random.default_rng(seed)
    opened = b.open([int(rng.integers(0, 1 << h)) for h in heights])
    b.deinit()
    roots = np.frombuffer(b"".join(r for r, _ in res), dtype=np.uint8).reshape(-1, 32).copy()
    leaves = np.array([o["value"] for o in opened], dtype=np.uint64)
    bad = rng.random(len(heights)) < 0.01
    leaves[bad] = (leaves[bad] + 1) % P
    return roots, leaves, [o["siblings"] for o in opened], [o["directions"] for o in opened]


def tile(pool, heights, k):
    """k openings: the pool's, repeated in order"""
    roots, leaves, sibs, dirs = pool
    n = len(heights)
    idx = np.arange(k) % n
    return Openings(roots[idx].reshape(-1), [heights[i] for i in idx], leaves[idx],
                    np.frombuffer(b"".join(sibs[i] for i in idx) + b"\0" * 32, dtype=np.uint8),
                    np.frombuffer(b"".join(dirs[i] for i in idx) + b"\0", dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two reps, no crossover (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = 2 if a.quick else a.reps
    import torch
    import zigz_amd
    from zigz_amd import host
    from zigz_amd._ffi import lib, u8p, u64p, vp
    import oracle_lib as O

    P = O.P_BB
    ctx = zigz_amd.Context(0)
    u8 = lambda x: x.ctypes.data_as(u8p)  # noqa: E731
    u64 = lambda x: x.ctypes.data_as(u64p)  # noqa: E731

    def host_verify(o):
        """zigzh_batch_verify over the openings (num_vars = height, zero points): verdict of the whole batch"""
        pts = np.zeros(max(sum(o.hlist), 1), dtype=np.uint64)
        z = np.zeros(o.k, dtype=np.uint64)
        ok = C.c_int(0)

        def run():
            rc = host.lib.zigzh_batch_verify(u8(o.roots), o.heights, o.k, u64(pts), u64(z), u64(z), u64(o.leaves), u8(o.sib),
                                             u8(o.dirs), C.byref(ok))
            assert rc == 0
            return ok.value
        return run

    def verify_call(o, dev):
        verd = np.zeros(o.k, dtype=np.uint8)
        rej, bad = C.c_size_t(0), C.c_size_t(0)

        def run():
            if dev:
                rc = lib.zigz_dev_merkle_verify_batch(ctx.h, o.k, vp(o.d[0].data_ptr()), o.heights, vp(o.d[1].data_ptr()),
                                                      vp(o.d[2].data_ptr()), vp(o.d[3].data_ptr()), u8(verd), C.byref(rej),
                                                      C.byref(bad))
            else:
                rc = lib.zigz_merkle_verify_batch(ctx.h, o.k, u8(o.roots), o.heights, u64(o.leaves), u8(o.sib), u8(o.dirs),
                                                  u8(verd), C.byref(rej), C.byref(bad))
            assert rc == 0
            return verd, rej.value
        return run

    def pause(mode):
        ctx.set_option("verify_pause", mode)

    def copy_call(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def run():
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
        return run

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

    out = {"reps": reps, "ceiling_perms_per_s": CEILING}
    pool20 = make_pool(ctx, P, [20] * 64, 100)
    mix_h = [h for h in range(25) for _ in range(4)]
    pool_mix = make_pool(ctx, P, mix_h, 200)
    shapes = [("43x20", [20] * 64, pool20, 43), ("4096x20", [20] * 64, pool20, 4096), ("2^16x20", [20] * 64, pool20, 1 << 16),
              ("2^20x20", [20] * 64, pool20, 1 << 20), ("mix_0..24_x2^16", mix_h, pool_mix, 1 << 16)]
    for name, hs, pool, k in shapes:
        o = tile(pool, hs, k)
        host_reps = reps if o.perms <= (1 << 22) else 3
        # verdicts: every form against the host's per-opening result (the host call gives only the batch verdict: check it and
        # the count of rejects against the pool's tampering)
        hv, hr = verify_call(o, False)()
        hv = hv.copy()
        dv, dr = verify_call(o, True)()
        assert np.array_equal(hv, dv) and hr == dr == int((hv == 0).sum())
        want = bool(host_verify(o)())
        assert want == (hr == 0)
        for i in np.random.default_rng(3).choice(k, size=min(k, 64), replace=False):
            h, off = o.hlist[i], sum(o.hlist[:i])
            assert bool(hv[i]) == host.batch_verify([(bytes(o.roots[32 * i:32 * i + 32]), h)], [dict(
                point=[0] * h, value=0, index=0, leaf=int(o.leaves[i]), siblings=bytes(o.sib[32 * off:32 * (off + h)]),
                directions=bytes(o.dirs[off:off + h]))]), (name, i)
        dcall = verify_call(o, True)
        t = timed({"hform": verify_call(o, False), "copy": copy_call(o.bytes),
                   "dform_pause": lambda: (pause(1), dcall()), "dform_nopause": lambda: (pause(2), dcall()),
                   "dform": lambda: (pause(0), dcall())}, reps)
        pause(0)
        th = timed({"host": host_verify(o)}, host_reps)["host"]
        r = dict(k=k, perms=o.perms, bytes=o.bytes, rejected=hr,
                 ms={f: round(v * 1e3, 4) for f, v in list(t.items()) + [("host", th)]})
        r["dform_Gperms_per_s"] = round(o.perms / t["dform"] / 1e9, 3)
        r["dform_of_ceiling"] = round(o.perms / t["dform"] / CEILING, 3)
        r["hform_over_copy"] = round(t["hform"] / t["copy"], 2)
        r["copy_GB_per_s"] = round(o.bytes / t["copy"] / 1e9, 2)
        r["host_Mperms_per_s"] = round(o.perms / th / 1e6, 2)
        r["dform_speedup_over_host"] = round(th / t["dform"], 1)
        r["hform_speedup_over_host"] = round(th / t["hform"], 1)
        r["pause_ab_ms"] = [round(t["dform_pause"] * 1e3, 4), round(t["dform_nopause"] * 1e3, 4)]
        out[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del o
    if not a.quick:
        cross = {}
        for k in (1, 4, 16, 43, 64, 128, 256, 512, 1024, 4096):
            o = tile(pool20, [20] * 64, k)
            t = timed({"host": host_verify(o), "hform": verify_call(o, False), "dform": verify_call(o, True)}, reps)
            cross[k] = {f: round(v * 1e6, 1) for f, v in t.items()}
            print("cross", k, cross[k], file=sys.stderr, flush=True)
        out["crossover_us_height20"] = cross
        out["crossover_k_host_faster_below"] = {
            f: next((k for k in sorted(cross) if cross[k][f] < cross[k]["host"]), None) for f in ("hform", "dform")}
    s = json.dumps(out)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
