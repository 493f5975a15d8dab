"""Python face of the C ABI (include/zigz_hip.h): a Context plus thin wrappers whose names and
argument meanings follow the reference types they stand in for -- Multilinear
(src/poly/multilinear.zig), SumcheckProver (src/proofs/sumcheck_prover.zig), SimpleMerkleTree
(src/commitments/merkle_tree.zig), CommitmentScheme (src/commitments/polynomial_commit.zig),
LassoProver (src/lookups/lasso_prover.zig).  All arithmetic happens in libzigz_hip.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import errors
from ._ffi import BenchResult, KernelStats, lib, u8p, u32p, u64p, vp

P = 2013265921
NUM_COLUMNS = 43
# zigz_trace_step (include/zigz_hip.h): one compact record per executed step, 48 bytes
TRACE_STEP_DTYPE = np.dtype([("pc", "<u8"), ("rd_value", "<u8"), ("mem_addr", "<u8"), ("mem_value", "<u8"), ("imm", "<i8"),
                             ("opcode", "u1"), ("rd", "u1"), ("rs1", "u1"), ("rs2", "u1"), ("funct3", "u1"), ("funct7", "u1"),
                             ("wr_reg", "u1"), ("mem_is_read", "u1")])
assert TRACE_STEP_DTYPE.itemsize == 48
# the 32-byte record and its side list (include/zigz_hip.h: zigz_trace_step32 / zigz_mem_access)
TRACE_STEP32_DTYPE = np.dtype([("pc", "<u8"), ("rd_value", "<u8"), ("imm", "<i4"), ("mem_index", "<u4"), ("opcode", "u1"), ("rd", "u1"),
                               ("rs1", "u1"), ("rs2", "u1"), ("funct3", "u1"), ("funct7", "u1"), ("wr_reg", "u1"), ("mem_is_read", "u1")])
MEM_ACCESS_DTYPE = np.dtype([("addr", "<u8"), ("value", "<u8")])
assert TRACE_STEP32_DTYPE.itemsize == 32 and MEM_ACCESS_DTYPE.itemsize == 16
NO_MEM_ACCESS = 0xFFFFFFFF
GRAND_PRODUCT_LEAF_DEFERRED = 1  # ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED: no column; A(leaf_point) == leaf_eval is the caller's check
SUMCHECK_VERIFY_POINT_REVERSED = 1  # ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED: the oracle at the reversed point (honest proofs accept)


def compact_steps32(steps, has_access):
    """48-byte records -> (32-byte records, side list): has_access[i] says whether step i has a memory access at all (a LOAD /
    STORE; its address and value may well be 0).  imm must fit 32 bits (it does in every RV64IM format)."""
    steps = np.ascontiguousarray(steps, dtype=TRACE_STEP_DTYPE)
    has_access = np.asarray(has_access, dtype=bool)
    out = np.zeros(len(steps), dtype=TRACE_STEP32_DTYPE)
    for f in ("pc", "rd_value", "opcode", "rd", "rs1", "rs2", "funct3", "funct7", "wr_reg", "mem_is_read"):
        out[f] = steps[f]
    assert np.all(steps["imm"] == steps["imm"].astype(np.int32)), "an immediate does not fit 32 bits"
    out["imm"] = steps["imm"].astype(np.int32)
    idx = np.flatnonzero(has_access)
    out["mem_index"] = NO_MEM_ACCESS
    out["mem_index"][idx] = np.arange(len(idx), dtype=np.uint32)
    mem = np.zeros(len(idx), dtype=MEM_ACCESS_DTYPE)
    mem["addr"], mem["value"] = steps["mem_addr"][idx], steps["mem_value"][idx]
    return out, mem


# the 16-byte record and the code table (include/zigz_hip.h: zigz_trace_step16 / zigz_code_entry)
TRACE_STEP16_DTYPE = np.dtype([("pc_word", "<u4"), ("mem_wr", "<u4"), ("rd_value", "<u8")])
CODE_ENTRY_DTYPE = np.dtype([("imm", "<i4"), ("opcode", "u1"), ("rd", "u1"), ("rs1", "u1"), ("rs2", "u1"), ("funct3", "u1"), ("funct7", "u1"),
                             ("reserved0", "u1"), ("reserved1", "u1")])
assert TRACE_STEP16_DTYPE.itemsize == 16 and CODE_ENTRY_DTYPE.itemsize == 12
NO_MEM_ACCESS16 = (1 << 27) - 1


def compact_steps16(steps, has_access):
    """48-byte records -> (16-byte records, side list, code_base, code table), or None when the trace does not fit the form (a pc off
    the 4-byte grid or 2^32 past the lowest one, one pc with two different decodings, 2^27 - 1 or more accesses)."""
    steps = np.ascontiguousarray(steps, dtype=TRACE_STEP_DTYPE)
    s32, mem = compact_steps32(steps, has_access)
    if len(steps) == 0 or len(mem) >= NO_MEM_ACCESS16:
        return None
    base = int(steps["pc"].min())
    off = steps["pc"] - np.uint64(base)
    if base & 3 or int(off.max()) >= 1 << 32 or np.any(off & np.uint64(3)) or np.any(steps["wr_reg"] >= 32) or np.any(steps["mem_is_read"] > 1):
        return None
    idx = (off >> np.uint64(2)).astype(np.int64)
    code = np.zeros(int(idx.max()) + 1, dtype=CODE_ENTRY_DTYPE)
    fields = ("imm", "opcode", "rd", "rs1", "rs2", "funct3", "funct7")
    first = {}
    for i in np.unique(idx, return_index=True)[1]:
        first[int(idx[i])] = int(i)
    for ci, i in first.items():
        for f in fields:
            code[f][ci] = s32[f][i]
    for f in fields:  # every step must agree with the entry of its pc
        if np.any(code[f][idx] != s32[f]):
            return None
    out = np.zeros(len(steps), dtype=TRACE_STEP16_DTYPE)
    out["pc_word"] = off.astype(np.uint32) | (steps["mem_is_read"].astype(np.uint32) & 1)
    mi = np.where(s32["mem_index"] == NO_MEM_ACCESS, np.uint32(NO_MEM_ACCESS16), s32["mem_index"]).astype(np.uint32)
    out["mem_wr"] = mi | (steps["wr_reg"].astype(np.uint32) << 27)
    out["rd_value"] = steps["rd_value"]
    return out, mem, base, code


def _name(code):
    return lib.zigz_status_name(code).decode()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        a = np.zeros(1, dtype=np.uint64)
    return a, a.ctypes.data_as(u64p)


def _out_u64(n):
    a = np.zeros(max(int(n), 1), dtype=np.uint64)
    return a, a.ctypes.data_as(u64p)


def _out_u8(n):
    a = np.zeros(max(int(n), 1), dtype=np.uint8)
    return a, a.ctypes.data_as(u8p)


def device_count():
    n = C.c_int(0)
    lib.zigz_device_count(C.byref(n))
    return n.value


class Context:
    """zigz_ctx: one HIP device + stream + workspace.  Raises ZigzError(NoDevice) without a gfx950 GPU."""

    def __init__(self, device=0, _borrowed=None):
        self.owned = _borrowed is None
        if _borrowed is not None:  # a context somebody else owns (a GPU slot of host.Slots): never destroyed from here
            self.h = _borrowed
            return
        h = vp()
        rc = lib.zigz_ctx_create(device, C.byref(h))
        if rc != 0:
            raise errors.ZigzError(rc, _name(rc), "zigz_ctx_create: a gfx950 (MI355X) device is required; no CPU fallback")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                lib.zigz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, rc):
        if rc != 0:
            raise errors.ZigzError(rc, _name(rc), lib.zigz_last_error(self.h).decode(errors="replace"))

    # ---- stream / memory
    def set_stream(self, hip_stream):
        self.check(lib.zigz_ctx_set_stream(self.h, vp(hip_stream) if hip_stream else None))

    def synchronize(self):
        self.check(lib.zigz_ctx_synchronize(self.h))

    def dev_alloc(self, nbytes):
        p = vp()
        self.check(lib.zigz_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        self.check(lib.zigz_dev_free(self.h, vp(ptr)))

    def upload(self, values, d_ptr):
        a, ap = _u64(values)
        self.check(lib.zigz_dev_upload_u64(self.h, ap, len(values), vp(d_ptr)))

    def reduce_upload(self, raw_u64, d_ptr):
        a, ap = _u64(raw_u64)
        self.check(lib.zigz_dev_reduce_u64(self.h, ap, len(raw_u64), vp(d_ptr)))

    def witness_from_rows(self, rows, nv, d_cols, stride):
        """WitnessGenerator.generate on the device from packed trace rows [num_steps, 43] (raw u64)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        self.check(lib.zigz_dev_witness_from_rows(self.h, rows.ctypes.data_as(u64p), rows.shape[0], nv, vp(d_cols), stride))

    def witness_from_steps(self, steps, nv, d_cols, stride, initial_regs=None):
        """WitnessGenerator.generate on the device from compact records (structured array of TRACE_STEP_DTYPE)."""
        steps = np.ascontiguousarray(steps, dtype=TRACE_STEP_DTYPE)
        ir = None
        if initial_regs is not None:
            ira = np.ascontiguousarray(initial_regs, dtype=np.uint64)
            assert ira.size == 32
            ir = ira.ctypes.data_as(u64p)
        self.check(lib.zigz_dev_witness_from_steps(self.h, vp(steps.ctypes.data), steps.shape[0], nv, ir, vp(d_cols), stride))

    def witness_from_steps32(self, steps32, mem, nv, d_cols, stride, initial_regs=None):
        """the same from the 32-byte records + side list of memory accesses (zigz_dev_witness_from_steps32)"""
        steps32 = np.ascontiguousarray(steps32, dtype=TRACE_STEP32_DTYPE)
        mem = np.ascontiguousarray(mem, dtype=MEM_ACCESS_DTYPE)
        ir = None
        if initial_regs is not None:
            ira = np.ascontiguousarray(initial_regs, dtype=np.uint64)
            assert ira.size == 32
            ir = ira.ctypes.data_as(u64p)
        self.check(lib.zigz_dev_witness_from_steps32(self.h, vp(steps32.ctypes.data), steps32.shape[0], vp(mem.ctypes.data) if len(mem) else None,
                                                     len(mem), nv, ir, vp(d_cols), stride))

    def witness_from_steps16(self, steps16, mem, code_base, code, nv, d_cols, stride, initial_regs=None):
        """the same from the 16-byte records + side list + code table (zigz_dev_witness_from_steps16)"""
        steps16 = np.ascontiguousarray(steps16, dtype=TRACE_STEP16_DTYPE)
        mem = np.ascontiguousarray(mem, dtype=MEM_ACCESS_DTYPE)
        code = np.ascontiguousarray(code, dtype=CODE_ENTRY_DTYPE)
        ir = None
        if initial_regs is not None:
            ira = np.ascontiguousarray(initial_regs, dtype=np.uint64)
            assert ira.size == 32
            ir = ira.ctypes.data_as(u64p)
        self.check(lib.zigz_dev_witness_from_steps16(self.h, vp(steps16.ctypes.data), steps16.shape[0], vp(mem.ctypes.data) if len(mem) else None,
                                                     len(mem), int(code_base), vp(code.ctypes.data) if len(code) else None, len(code), nv, ir,
                                                     vp(d_cols), stride))

    def download(self, d_ptr, n):
        o, op = _out_u64(n)
        self.check(lib.zigz_dev_download_u64(self.h, vp(d_ptr), n, op))
        return o[:n]

    def enable_timing(self, on=True):
        self.check(lib.zigz_ctx_enable_timing(self.h, 1 if on else 0))

    def set_option(self, name, value):
        self.check(lib.zigz_ctx_set_option(self.h, name.encode(), int(value)))

    def release_workspaces(self):
        """give the context's workspaces back to the device (they regrow on demand)"""
        self.check(lib.zigz_ctx_release_workspaces(self.h))

    def mem_info(self):
        """(free, total) bytes of HBM on this context's device"""
        f, t = C.c_size_t(), C.c_size_t()
        self.check(lib.zigz_dev_mem_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def get_option(self, name):
        v = C.c_int64()
        self.check(lib.zigz_ctx_get_option(self.h, name.encode(), C.byref(v)))
        return v.value & 0xFFFFFFFFFFFFFFFF

    def stats(self):
        s = KernelStats()
        self.check(lib.zigz_ctx_get_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in KernelStats._fields_}

    def set_epoch(self, owner=None):
        """zigz_ctx_set_epoch: a new epoch of this context's (owner None) or the adoption of another context's: what the
        times of launch_log() count from."""
        self.check(lib.zigz_ctx_set_epoch(self.h, (owner or self).h))

    def launch_log(self):
        """zigz_ctx_launch_log: [(class, permutations, start_us, end_us)] of the timed launches of the last commit job."""
        from ._ffi import LaunchRec
        buf = (LaunchRec * 80)()
        n = C.c_size_t()
        self.check(lib.zigz_ctx_launch_log(self.h, buf, 80, C.byref(n)))
        return [(buf[i].cls, buf[i].perms, buf[i].start_us, buf[i].end_us) for i in range(min(n.value, 80))]

    def bench_kernel(self, kernel, nv, ncols, iters=10, cold=True):
        """zigz_bench_kernel: per-launch kernel durations of one hot kernel on a synthetic resident table."""
        r = BenchResult()
        self.check(lib.zigz_bench_kernel(self.h, kernel.encode(), nv, ncols, iters, 1 if cold else 0, C.byref(r)))
        return {f: getattr(r, f) for f, _ in BenchResult._fields_}

    # ---- Multilinear(F) seams, host buffers
    def mle_bind(self, evals, r):
        """partialEval(self, r), multilinear.zig:154"""
        a, ap = _u64(evals)
        o, op = _out_u64(len(evals) // 2)
        self.check(lib.zigz_mle_bind(self.h, ap, len(evals), int(r), op))
        return o[: len(evals) // 2]

    def mle_round_poly(self, evals):
        """roundPolynomial(self), multilinear.zig:205"""
        a, ap = _u64(evals)
        o, op = _out_u64(2)
        self.check(lib.zigz_mle_round_poly(self.h, ap, len(evals), op))
        return [int(o[0]), int(o[1])]

    def mle_sum(self, evals):
        """sumOverHypercube(self), multilinear.zig:188"""
        a, ap = _u64(evals)
        out = C.c_uint64()
        self.check(lib.zigz_mle_sum(self.h, ap, len(evals), C.byref(out)))
        return out.value

    def mle_eval(self, evals, point):
        """eval(self, point), multilinear.zig:110"""
        a, ap = _u64(evals)
        q, qp = _u64(point)
        out = C.c_uint64()
        self.check(lib.zigz_mle_eval(self.h, ap, len(evals), qp, len(point), C.byref(out)))
        return out.value

    # ---- SumcheckProver(F)
    def sumcheck_prove(self, evals, challenges=None):
        """prove(poly) / proveInteractive(poly, challenges), sumcheck_prover.zig:26,97.
        Returns (rounds[2v], final_point[v], final_eval)."""
        a, ap = _u64(evals)
        n = len(evals)
        nv = max(n.bit_length() - 1, 0)
        r, rp = _out_u64(2 * nv)
        pt, ptp = _out_u64(nv)
        fe = C.c_uint64()
        if challenges is None:
            self.check(lib.zigz_sumcheck_prove(self.h, ap, n, rp, ptp, C.byref(fe)))
        else:
            c, cp = _u64(challenges)
            self.check(lib.zigz_sumcheck_prove_interactive(self.h, ap, n, cp, len(challenges), rp, ptp, C.byref(fe)))
        return r[: 2 * nv].copy(), pt[:nv].copy(), fe.value

    # ---- device-resident variants (packed u32 canonical in HBM)
    def dev_mle_bind(self, d_in, n, r, d_out):
        self.check(lib.zigz_dev_mle_bind(self.h, vp(d_in), n, int(r), vp(d_out)))

    def dev_mle_bind_sums(self, d_in, n, r, d_out):
        o, op = _out_u64(2)
        self.check(lib.zigz_dev_mle_bind_sums(self.h, vp(d_in), n, int(r), vp(d_out), op))
        return [int(o[0]), int(o[1])]

    def dev_mle_half_sums(self, d_in, n):
        o, op = _out_u64(2)
        self.check(lib.zigz_dev_mle_half_sums(self.h, vp(d_in), n, op))
        return [int(o[0]), int(o[1])]

    def dev_mle_eval(self, d_in, n, point):
        q, qp = _u64(point)
        out = C.c_uint64()
        self.check(lib.zigz_dev_mle_eval(self.h, vp(d_in), n, qp, len(point), C.byref(out)))
        return out.value

    def dev_sumcheck_prove(self, d_in, n, challenges=None, d_scratch=None):
        nv = max(n.bit_length() - 1, 0)
        r, rp = _out_u64(2 * nv)
        pt, ptp = _out_u64(nv)
        fe = C.c_uint64()
        cp = None
        if challenges is not None:
            c, cp = _u64(challenges)
        self.check(lib.zigz_dev_sumcheck_prove(self.h, vp(d_in), n, vp(d_scratch) if d_scratch else None, cp, rp, ptp,
                                               C.byref(fe)))
        return r[: 2 * nv].copy(), pt[:nv].copy(), fe.value

    def dev_sumcheck_prove_sharded(self, d_local, n_local, rank, world, allgather, user=None):
        """zigz_dev_sumcheck_prove_sharded: SumcheckProver.prove of ONE table sharded by rows (element i on rank i mod world
        at local index i // world).  `allgather`: an _ffi.ALLGATHER_FN (shard.make_allgather(dist))."""
        nv = (n_local * world).bit_length() - 1
        r, rp = _out_u64(2 * nv)
        pt, ptp = _out_u64(nv)
        fe = C.c_uint64()
        self.check(lib.zigz_dev_sumcheck_prove_sharded(self.h, vp(d_local), n_local, rank, world, allgather, user, rp, ptp,
                                                       C.byref(fe)))
        return r[: 2 * nv].copy(), pt[:nv].copy(), fe.value

    def dev_sumcheck_prove_rccl(self, d_local, n_local, comm):
        """zigz_dev_sumcheck_prove_rccl: the same proof with a shard.RcclComm as the transport -- the partial block sums of
        every radix stage are all-reduced in HBM on this context's stream, the tail all-gathered through the comm."""
        nv = (n_local * comm.world).bit_length() - 1
        r, rp = _out_u64(2 * nv)
        pt, ptp = _out_u64(nv)
        fe = C.c_uint64()
        self.check(lib.zigz_dev_sumcheck_prove_rccl(self.h, vp(d_local), n_local, comm.h, rp, ptp, C.byref(fe)))
        return r[: 2 * nv].copy(), pt[:nv].copy(), fe.value

    # ---- batched provers (k independent tables per call, shared launches)
    def check_batch(self, rc, bad):
        """check() for the batch entries: the exception carries the index of the first failing table as .bad_index"""
        if rc != 0:
            e = errors.ZigzError(rc, _name(rc), lib.zigz_last_error(self.h).decode(errors="replace"))
            e.bad_index = bad.value
            raise e

    @staticmethod
    def _batch_out(ns):
        nvs = [max(int(n).bit_length() - 1, 0) for n in ns]
        tot = sum(nvs)
        r, rp = _out_u64(2 * tot)
        pt, ptp = _out_u64(tot)
        fe, fep = _out_u64(len(ns))
        return nvs, (r, rp), (pt, ptp), (fe, fep)

    @staticmethod
    def _batch_split(nvs, r, pt, fe):
        out, o = [], 0
        for i, v in enumerate(nvs):
            out.append((r[2 * o: 2 * (o + v)].copy(), pt[o: o + v].copy(), int(fe[i])))
            o += v
        return out

    def sumcheck_prove_batch(self, tables, challenges=None):
        """zigz_sumcheck_prove_batch: sumcheck_prove(t[, challenges[i]]) for every table, in shared launches.
        Returns the list of (rounds, point, final_eval)."""
        k = len(tables)
        arrs = [_u64(t) for t in tables]
        ns = (C.c_size_t * max(k, 1))(*[len(t) for t in tables])
        ptrs = (u64p * max(k, 1))(*[p for _, p in arrs])
        nvs, (r, rp), (pt, ptp), (fe, fep) = self._batch_out([len(t) for t in tables])
        cp = None
        if challenges is not None:
            c, cp = _u64(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in challenges] + [np.zeros(0, np.uint64)]))
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_sumcheck_prove_batch(self.h, ptrs, ns, k, cp, rp, ptp, fep, C.byref(bad)), bad)
        return self._batch_split(nvs, r, pt, fe)

    def dev_sumcheck_prove_batch(self, d_tables, ns, challenges=None):
        """zigz_dev_sumcheck_prove_batch over device-resident tables (packed u32 canonical, 16-byte aligned)."""
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        ptrs = (vp * max(k, 1))(*[int(d) for d in d_tables])
        nvs, (r, rp), (pt, ptp), (fe, fep) = self._batch_out(ns)
        cp = None
        if challenges is not None:
            c, cp = _u64(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in challenges] + [np.zeros(0, np.uint64)]))
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_dev_sumcheck_prove_batch(self.h, ptrs, nsa, k, cp, rp, ptp, fep, C.byref(bad)), bad)
        return self._batch_split(nvs, r, pt, fe)

    # ---- batched MLE evaluation and sumcheck verification (k independent pairs / proofs per call, one eval launch)
    @staticmethod
    def _cat_u64(parts):
        return _u64(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in parts] + [np.zeros(1, np.uint64)]))

    def mle_eval_batch(self, tables, points):
        """zigz_mle_eval_batch: mle_eval(tables[i], points[i]) for every pair, in shared launches.  Returns the k values."""
        k = len(tables)
        arrs = [_u64(t) for t in tables]
        ns = (C.c_size_t * max(k, 1))(*[len(t) for t in tables])
        ptrs = (u64p * max(k, 1))(*[p for _, p in arrs])
        q, qp = self._cat_u64(points)
        o, op = _out_u64(k)
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_mle_eval_batch(self.h, ptrs, ns, k, qp, op, C.byref(bad)), bad)
        return [int(x) for x in o[:k]]

    def dev_mle_eval_batch(self, d_tables, ns, points):
        """zigz_dev_mle_eval_batch over device-resident tables (packed u32 canonical, 16-byte aligned); points[i] has
        log2(ns[i]) coordinates."""
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        ptrs = (vp * max(k, 1))(*[int(d) for d in d_tables])
        q, qp = self._cat_u64(points)
        o, op = _out_u64(k)
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_dev_mle_eval_batch(self.h, ptrs, nsa, k, qp, op, C.byref(bad)), bad)
        return [int(x) for x in o[:k]]

    def _sumcheck_verify_batch(self, fn, ptrs, ns, claimed_sums, proofs, flags):
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        cs, csp = self._cat_u64([claimed_sums])
        r, rp = self._cat_u64([p[0] for p in proofs])
        q, qp = self._cat_u64([p[1] for p in proofs])
        fe, fep = self._cat_u64([[int(p[2]) for p in proofs]])
        verd, vdp = _out_u8(k)
        exp, ep = _out_u64(k)
        orc, op = _out_u64(k)
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        self.check_batch(fn(self.h, ptrs, nsa, k, csp, rp, qp, fep, int(flags), vdp, ep, op, C.byref(rej), C.byref(bad)), bad)
        return verd[:k].copy(), [int(x) for x in exp[:k]], [int(x) for x in orc[:k]], rej.value

    def sumcheck_verify_batch(self, tables, claimed_sums, proofs, flags=0):
        """zigz_sumcheck_verify_batch: SumcheckVerifier.verify of proofs[i] = (rounds, point, final_eval) against claimed_sums[i],
        the oracle being table i's multilinear extension.  flags: 0 evaluates at the point as given (the reference: honest
        proofs of two or more variables are rejected in general), SUMCHECK_VERIFY_POINT_REVERSED at the reversed point (honest
        proofs accept).  Returns (verdicts np.uint8, expected_evals, oracle_evals, n_rejected)."""
        k = len(tables)
        arrs = [_u64(t) for t in tables]
        ptrs = (u64p * max(k, 1))(*[p for _, p in arrs])
        return self._sumcheck_verify_batch(lib.zigz_sumcheck_verify_batch, ptrs, [len(t) for t in tables], claimed_sums, proofs, flags)

    def dev_sumcheck_verify_batch(self, d_tables, ns, claimed_sums, proofs, flags=0):
        """zigz_dev_sumcheck_verify_batch over device-resident tables (packed u32 canonical, 16-byte aligned)."""
        ptrs = (vp * max(len(ns), 1))(*[int(d) for d in d_tables])
        return self._sumcheck_verify_batch(lib.zigz_dev_sumcheck_verify_batch, ptrs, ns, claimed_sums, proofs, flags)

    # ---- batched product sumcheck prover (k independent sums of products of 1..3 tables per call, one data pass per round)
    def _product_batch(self, fn, ptrs, degrees, ns, challenges):
        k = len(ns)
        nvs = [max(int(n).bit_length() - 1, 0) for n in ns]
        nf = max(sum(degrees), 1)
        dg = (C.c_uint * max(k, 1))(*[int(d) for d in degrees])
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        cs, csp = _out_u64(k)
        r, rp = _out_u64(sum((d + 1) * v for d, v in zip(degrees, nvs)))
        pt, ptp = _out_u64(sum(nvs))
        fv, fvp = _out_u64(nf)
        fe, fep = _out_u64(k)
        cp = None
        if challenges is not None:
            c, cp = self._cat_u64(challenges)
        bad = C.c_size_t(0)
        self.check_batch(fn(self.h, k, dg, ptrs, nsa, cp, csp, rp, ptp, fvp, fep, C.byref(bad)), bad)
        out, ro, vo, fo = [], 0, 0, 0
        for i, (d, v) in enumerate(zip(degrees, nvs)):
            out.append((int(cs[i]), r[ro: ro + (d + 1) * v].copy(), pt[vo: vo + v].copy(), fv[fo: fo + d].copy(), int(fe[i])))
            ro, vo, fo = ro + (d + 1) * v, vo + v, fo + d
        return out

    def sumcheck_prove_product_batch(self, instances, challenges=None):
        """zigz_sumcheck_prove_product_batch: instances[i] is the list of 1..3 equally long tables whose product is summed;
        challenges[i] (optional) fixes instance i's challenges (the interactive form, no transcript).  Returns per instance
        (claimed_sum, rounds [(d + 1) words c_0..c_d per round], point, factor_evals [d], final_eval)."""
        arrs = [_u64(t) for inst in instances for t in inst]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        return self._product_batch(lib.zigz_sumcheck_prove_product_batch, ptrs, [len(inst) for inst in instances],
                                   [len(inst[0]) if len(inst) else 0 for inst in instances], challenges)

    def dev_sumcheck_prove_product_batch(self, d_instances, ns, challenges=None):
        """zigz_dev_sumcheck_prove_product_batch: d_instances[i] is the list of instance i's 1..3 device tables (packed u32
        canonical, 16-byte aligned, ns[i] values each; read only -- the same pointer may repeat)."""
        flat = [int(d) for inst in d_instances for d in inst]
        ptrs = (vp * max(len(flat), 1))(*flat)
        return self._product_batch(lib.zigz_dev_sumcheck_prove_product_batch, ptrs, [len(inst) for inst in d_instances], ns, challenges)

    # ---- batched eq tables and the verification of product proofs (a zero-check end to end: DESIGN.md s7h)
    def eq_table_batch(self, ns, points):
        """zigz_eq_table_batch: for every i the table E[x] = prod_j (bit j of x ? tau_j : 1 - tau_j) of ns[i] = 2^v canonical
        words, tau = points[i] (v coordinates, tau[0] with the LSB of x).  Returns the list of np.uint64 arrays."""
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        q, qp = self._cat_u64(points)
        outs = [_out_u64(n) for n in ns]
        ptrs = (u64p * max(k, 1))(*[p for _, p in outs])
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_eq_table_batch(self.h, k, nsa, qp, ptrs, C.byref(bad)), bad)
        return [o[:int(n)] for (o, _), n in zip(outs, ns)]

    def dev_eq_table_batch(self, d_out, ns, points):
        """zigz_dev_eq_table_batch into device memory (addresses, 16-byte aligned, ns[i] u32 words each): queued on the context's
        stream, not waited for."""
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        ptrs = (vp * max(k, 1))(*[int(d) for d in d_out])
        q, qp = self._cat_u64(points)
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_dev_eq_table_batch(self.h, k, nsa, qp, ptrs, C.byref(bad)), bad)

    def _verify_product_batch(self, fn, ptrs, degrees, kinds, taus, ns, proofs, flags, check_factor_evals):
        k = len(ns)
        dg = (C.c_uint * max(k, 1))(*[int(d) for d in degrees])
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        kp = None
        if kinds is not None:
            kn = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint8).reshape(-1) for x in kinds] + [np.zeros(1, np.uint8)]))
            kp = kn.ctypes.data_as(u8p)
        tp = None
        if taus is not None:
            tq, tp = self._cat_u64(taus)
        cs, csp = self._cat_u64([[int(p[0]) for p in proofs]])
        r, rp = self._cat_u64([p[1] for p in proofs])
        q, qp = self._cat_u64([p[2] for p in proofs])
        fv, fvp = self._cat_u64([p[3] for p in proofs])
        fe, fep = self._cat_u64([[int(p[4]) for p in proofs]])
        nf = sum(int(d) for d in degrees)
        verd, vdp = _out_u8(k)
        exp, ep = _out_u64(k)
        orc, op = _out_u64(nf)
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        self.check_batch(fn(self.h, k, dg, ptrs, kp, tp, nsa, csp, rp, qp, fvp if check_factor_evals else None, fep, int(flags), vdp, ep,
                            op, C.byref(rej), C.byref(bad)), bad)
        oracle, o = [], 0
        for d in degrees:
            oracle.append([int(x) for x in orc[o: o + int(d)]])
            o += int(d)
        return verd[:k].copy(), [int(x) for x in exp[:k]], oracle, rej.value

    def sumcheck_verify_product_batch(self, instances, proofs, flags=0, taus=None, check_factor_evals=True):
        """zigz_sumcheck_verify_product_batch: proofs[i] = (claimed_sum, rounds, point, factor_evals, final_eval) as
        sumcheck_prove_product_batch returns it, instances[i] the list of its 1..3 factors -- a table, or None for eq(tau, .),
        whose tau is the next entry of `taus`.  flags as sumcheck_verify_batch's.  check_factor_evals=False passes
        factor_evals = NULL.  Returns (verdicts np.uint8, expected_evals, oracle_evals [d per proof], n_rejected)."""
        arrs = [(None, None) if t is None else _u64(t) for inst in instances for t in inst]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        kinds = [[1 if t is None else 0 for t in inst] for inst in instances]
        ns = [1 << len(p[2]) if all(t is None for t in inst) else len(next(t for t in inst if t is not None))
              for inst, p in zip(instances, proofs)]
        return self._verify_product_batch(lib.zigz_sumcheck_verify_product_batch, ptrs, [len(inst) for inst in instances], kinds, taus,
                                          ns, proofs, flags, check_factor_evals)

    def dev_sumcheck_verify_product_batch(self, d_instances, ns, proofs, flags=0, taus=None, check_factor_evals=True):
        """zigz_dev_sumcheck_verify_product_batch: d_instances[i] lists proof i's factors as device addresses (packed u32
        canonical, 16-byte aligned, ns[i] values), None for eq(tau, .)."""
        flat = [d for inst in d_instances for d in inst]
        ptrs = (vp * max(len(flat), 1))(*[None if d is None else int(d) for d in flat])
        kinds = [[1 if d is None else 0 for d in inst] for inst in d_instances]
        return self._verify_product_batch(lib.zigz_dev_sumcheck_verify_product_batch, ptrs, [len(inst) for inst in d_instances], kinds,
                                          taus, ns, proofs, flags, check_factor_evals)

    # ---- batched sum-of-products sumcheck: a pool of tables and terms alpha * prod pool[idx] per instance
    @staticmethod
    def _sop_terms(all_terms):
        """the flat term arrays of the entries: (n_terms, term_degrees, term_tables, term_coeffs) and the ctypes views that own them"""
        k = len(all_terms)
        nt = (C.c_uint * max(k, 1))(*[len(terms) for terms in all_terms])
        flat = [(int(alpha), [int(x) for x in idx]) for terms in all_terms for alpha, idx in terms]
        dg = (C.c_uint * max(len(flat), 1))(*[len(idx) for _, idx in flat])
        ix = np.array([x for _, idx in flat for x in idx] + [0], dtype=np.uint8)
        co, cop = _u64(np.array([alpha for alpha, _ in flat] + [0], dtype=np.uint64))
        return nt, dg, (ix, ix.ctypes.data_as(u8p)), (co, cop)

    @staticmethod
    def _sop_degrees(all_terms):
        return [max([len(idx) for _, idx in terms] + [0]) for terms in all_terms]

    def _sop_batch(self, fn, ptrs, pool_sizes, all_terms, ns, challenges):
        k = len(ns)
        nvs = [max(int(n).bit_length() - 1, 0) for n in ns]
        degrees = self._sop_degrees(all_terms)
        nm = (C.c_uint * max(k, 1))(*[int(m) for m in pool_sizes])
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        nt, dg, (ix, ixp), (co, cop) = self._sop_terms(all_terms)
        cs, csp = _out_u64(k)
        r, rp = _out_u64(sum((d + 1) * v for d, v in zip(degrees, nvs)))
        pt, ptp = _out_u64(sum(nvs))
        tv, tvp = _out_u64(sum(pool_sizes))
        fe, fep = _out_u64(k)
        cp = None
        if challenges is not None:
            c, cp = self._cat_u64(challenges)
        bad = C.c_size_t(0)
        self.check_batch(fn(self.h, k, nm, ptrs, nsa, nt, dg, ixp, cop, cp, csp, rp, ptp, tvp, fep, C.byref(bad)), bad)
        out, ro, vo, mo = [], 0, 0, 0
        for i, (d, v, m) in enumerate(zip(degrees, nvs, pool_sizes)):
            out.append((int(cs[i]), r[ro: ro + (d + 1) * v].copy(), pt[vo: vo + v].copy(), tv[mo: mo + m].copy(), int(fe[i])))
            ro, vo, mo = ro + (d + 1) * v, vo + v, mo + m
        return out

    def sumcheck_prove_sop_batch(self, instances, challenges=None):
        """zigz_sumcheck_prove_sop_batch: instances[i] = (tables, terms) -- a pool of 1..8 equally long tables and 1..8 terms
        (alpha, (idx, ...)), each a coefficient times the product of 1..3 pool tables named by index; the instance proves
        sum_x sum_t alpha_t prod_j tables[idx_j](x).  challenges[i] (optional) fixes instance i's challenges.  Returns per
        instance (claimed_sum, rounds [(D + 1) words per round, D the largest term degree], point, table_evals [one per pool
        table], final_eval)."""
        arrs = [_u64(t) for tables, _ in instances for t in tables]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        return self._sop_batch(lib.zigz_sumcheck_prove_sop_batch, ptrs, [len(tables) for tables, _ in instances],
                               [terms for _, terms in instances], [len(tables[0]) if len(tables) else 0 for tables, _ in instances],
                               challenges)

    def dev_sumcheck_prove_sop_batch(self, d_instances, ns, challenges=None):
        """zigz_dev_sumcheck_prove_sop_batch: d_instances[i] = (device tables, terms), the tables packed u32 canonical, 16-byte
        aligned, ns[i] values each; read only."""
        flat = [int(d) for tables, _ in d_instances for d in tables]
        ptrs = (vp * max(len(flat), 1))(*flat)
        return self._sop_batch(lib.zigz_dev_sumcheck_prove_sop_batch, ptrs, [len(tables) for tables, _ in d_instances],
                               [terms for _, terms in d_instances], ns, challenges)

    def _verify_sop_batch(self, fn, ptrs, pool_sizes, kinds, taus, all_terms, ns, proofs, flags, check_table_evals):
        k = len(ns)
        nm = (C.c_uint * max(k, 1))(*[int(m) for m in pool_sizes])
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        nt, dg, (ix, ixp), (co, cop) = self._sop_terms(all_terms)
        kn = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint8).reshape(-1) for x in kinds] + [np.zeros(1, np.uint8)]))
        tp = None
        if taus is not None:
            tq, tp = self._cat_u64(taus)
        cs, csp = self._cat_u64([[int(p[0]) for p in proofs]])
        r, rp = self._cat_u64([p[1] for p in proofs])
        q, qp = self._cat_u64([p[2] for p in proofs])
        tv, tvp = self._cat_u64([p[3] for p in proofs])
        fe, fep = self._cat_u64([[int(p[4]) for p in proofs]])
        verd, vdp = _out_u8(k)
        exp, ep = _out_u64(k)
        orc, op = _out_u64(sum(pool_sizes))
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        self.check_batch(fn(self.h, k, nm, ptrs, kn.ctypes.data_as(u8p), tp, nsa, nt, dg, ixp, cop, csp, rp, qp,
                            tvp if check_table_evals else None, fep, int(flags), vdp, ep, op, C.byref(rej), C.byref(bad)), bad)
        oracle, o = [], 0
        for m in pool_sizes:
            oracle.append([int(x) for x in orc[o: o + m]])
            o += m
        return verd[:k].copy(), [int(x) for x in exp[:k]], oracle, rej.value

    def sumcheck_verify_sop_batch(self, instances, proofs, flags=0, taus=None, check_table_evals=True):
        """zigz_sumcheck_verify_sop_batch: proofs[i] = (claimed_sum, rounds, point, table_evals, final_eval) as
        sumcheck_prove_sop_batch returns it, instances[i] = (pool, terms) with a pool entry a table, or None for eq(tau, .), whose
        tau is the next entry of `taus`.  flags as sumcheck_verify_batch's.  Returns (verdicts np.uint8, expected_evals,
        oracle_evals [one per pool entry and proof], n_rejected)."""
        arrs = [(None, None) if t is None else _u64(t) for tables, _ in instances for t in tables]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        kinds = [[1 if t is None else 0 for t in tables] for tables, _ in instances]
        ns = [1 << len(p[2]) if all(t is None for t in tables) else len(next(t for t in tables if t is not None))
              for (tables, _), p in zip(instances, proofs)]
        return self._verify_sop_batch(lib.zigz_sumcheck_verify_sop_batch, ptrs, [len(tables) for tables, _ in instances], kinds, taus,
                                      [terms for _, terms in instances], ns, proofs, flags, check_table_evals)

    def dev_sumcheck_verify_sop_batch(self, d_instances, ns, proofs, flags=0, taus=None, check_table_evals=True):
        """zigz_dev_sumcheck_verify_sop_batch: d_instances[i] = (pool, terms), the pool's entries device addresses (packed u32
        canonical, 16-byte aligned, ns[i] values) or None for eq(tau, .)."""
        flat = [d for tables, _ in d_instances for d in tables]
        ptrs = (vp * max(len(flat), 1))(*[None if d is None else int(d) for d in flat])
        kinds = [[1 if d is None else 0 for d in tables] for tables, _ in d_instances]
        return self._verify_sop_batch(lib.zigz_dev_sumcheck_verify_sop_batch, ptrs, [len(tables) for tables, _ in d_instances], kinds,
                                      taus, [terms for _, terms in d_instances], ns, proofs, flags, check_table_evals)

    # ---- zero-check with the eq factor in closed form: a pool WITHOUT eq, terms of degree 1..3 and tau per instance
    def _zerocheck_batch(self, fn, ptrs, pool_sizes, all_terms, taus, ns, challenges):
        k = len(ns)
        nvs = [max(int(n).bit_length() - 1, 0) for n in ns]
        degrees = self._sop_degrees(all_terms)
        nm = (C.c_uint * max(k, 1))(*[int(m) for m in pool_sizes])
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        nt, dg, (ix, ixp), (co, cop) = self._sop_terms(all_terms)
        tq, tp = self._cat_u64(taus)
        cs, csp = _out_u64(k)
        r, rp = _out_u64(sum((d + 2) * v for d, v in zip(degrees, nvs)))
        pt, ptp = _out_u64(sum(nvs))
        tv, tvp = _out_u64(sum(pool_sizes))
        ee, eep = _out_u64(k)
        fe, fep = _out_u64(k)
        cp = None
        if challenges is not None:
            c, cp = self._cat_u64(challenges)
        bad = C.c_size_t(0)
        self.check_batch(fn(self.h, k, nm, ptrs, nsa, nt, dg, ixp, cop, tp, cp, csp, rp, ptp, tvp, eep, fep, C.byref(bad)), bad)
        out, ro, vo, mo = [], 0, 0, 0
        for i, (d, v, m) in enumerate(zip(degrees, nvs, pool_sizes)):
            out.append((int(cs[i]), r[ro: ro + (d + 2) * v].copy(), pt[vo: vo + v].copy(), tv[mo: mo + m].copy(), int(ee[i]), int(fe[i])))
            ro, vo, mo = ro + (d + 2) * v, vo + v, mo + m
        return out

    def sumcheck_prove_zerocheck_batch(self, instances, challenges=None):
        """zigz_sumcheck_prove_zerocheck_batch: instances[i] = (tables, terms, tau) -- a pool of 1..8 equally long tables (none of
        them eq), 1..8 terms (alpha, (idx, ...)) of degree 1..3 as sumcheck_prove_sop_batch takes them, and tau (log2 n canonical
        words, tau[0] with the LSB); the instance proves sum_x eq(tau, x) sum_t alpha_t prod_j tables[idx_j](x) without an eq
        table.  Returns per instance (claimed_sum, rounds [(D + 2) words per round, D the largest term degree], point,
        table_evals [one per pool table], eq_eval, final_eval)."""
        arrs = [_u64(t) for tables, _, _ in instances for t in tables]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        return self._zerocheck_batch(lib.zigz_sumcheck_prove_zerocheck_batch, ptrs, [len(tables) for tables, _, _ in instances],
                                     [terms for _, terms, _ in instances], [tau for _, _, tau in instances],
                                     [len(tables[0]) if len(tables) else 0 for tables, _, _ in instances], challenges)

    def dev_sumcheck_prove_zerocheck_batch(self, d_instances, ns, challenges=None):
        """zigz_dev_sumcheck_prove_zerocheck_batch: d_instances[i] = (device tables, terms, tau), the tables packed u32 canonical,
        16-byte aligned, ns[i] values each; read only."""
        flat = [int(d) for tables, _, _ in d_instances for d in tables]
        ptrs = (vp * max(len(flat), 1))(*flat)
        return self._zerocheck_batch(lib.zigz_dev_sumcheck_prove_zerocheck_batch, ptrs, [len(tables) for tables, _, _ in d_instances],
                                     [terms for _, terms, _ in d_instances], [tau for _, _, tau in d_instances], ns, challenges)

    def _verify_zerocheck_batch(self, fn, ptrs, pool_sizes, all_terms, taus, ns, proofs, flags, check_table_evals, check_eq_evals):
        k = len(ns)
        nm = (C.c_uint * max(k, 1))(*[int(m) for m in pool_sizes])
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        nt, dg, (ix, ixp), (co, cop) = self._sop_terms(all_terms)
        tq, tp = self._cat_u64(taus)
        cs, csp = self._cat_u64([[int(p[0]) for p in proofs]])
        r, rp = self._cat_u64([p[1] for p in proofs])
        q, qp = self._cat_u64([p[2] for p in proofs])
        tv, tvp = self._cat_u64([p[3] for p in proofs])
        ee, eep = self._cat_u64([[int(p[4]) for p in proofs]])
        fe, fep = self._cat_u64([[int(p[5]) for p in proofs]])
        verd, vdp = _out_u8(k)
        exp, ep = _out_u64(k)
        orc, op = _out_u64(sum(pool_sizes))
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        self.check_batch(fn(self.h, k, nm, ptrs, tp, nsa, nt, dg, ixp, cop, csp, rp, qp, tvp if check_table_evals else None,
                            eep if check_eq_evals else None, fep, int(flags), vdp, ep, op, C.byref(rej), C.byref(bad)), bad)
        oracle, o = [], 0
        for m in pool_sizes:
            oracle.append([int(x) for x in orc[o: o + m]])
            o += m
        return verd[:k].copy(), [int(x) for x in exp[:k]], oracle, rej.value

    def sumcheck_verify_zerocheck_batch(self, instances, proofs, flags=0, check_table_evals=True, check_eq_evals=True):
        """zigz_sumcheck_verify_zerocheck_batch: proofs[i] = (claimed_sum, rounds, point, table_evals, eq_eval, final_eval) as
        sumcheck_prove_zerocheck_batch returns it, instances[i] = (tables, terms, tau).  flags as sumcheck_verify_batch's.
        Returns (verdicts np.uint8, expected_evals, oracle_evals [one per pool table and proof], n_rejected)."""
        arrs = [_u64(t) for tables, _, _ in instances for t in tables]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        return self._verify_zerocheck_batch(lib.zigz_sumcheck_verify_zerocheck_batch, ptrs, [len(tables) for tables, _, _ in instances],
                                            [terms for _, terms, _ in instances], [tau for _, _, tau in instances],
                                            [len(tables[0]) if len(tables) else 0 for tables, _, _ in instances], proofs, flags,
                                            check_table_evals, check_eq_evals)

    def dev_sumcheck_verify_zerocheck_batch(self, d_instances, ns, proofs, flags=0, check_table_evals=True, check_eq_evals=True):
        """zigz_dev_sumcheck_verify_zerocheck_batch: d_instances[i] = (device tables, terms, tau), the tables packed u32 canonical,
        16-byte aligned, ns[i] values each."""
        flat = [d for tables, _, _ in d_instances for d in tables]
        ptrs = (vp * max(len(flat), 1))(*[None if d is None else int(d) for d in flat])
        return self._verify_zerocheck_batch(lib.zigz_dev_sumcheck_verify_zerocheck_batch, ptrs,
                                            [len(tables) for tables, _, _ in d_instances], [terms for _, terms, _ in d_instances],
                                            [tau for _, _, tau in d_instances], ns, proofs, flags, check_table_evals, check_eq_evals)

    # ---- product trees and the grand-product argument
    def product_layers_batch(self, tables):
        """zigz_product_layers_batch: for every column (2^v canonical words) its product tree as one np.uint64 array of n words --
        layer j (2^j words) at word n - 2^(j+1), j = v - 1 .. 0, the product at word n - 2; word n - 1 is not written (left 0)."""
        k = len(tables)
        arrs = [_u64(t) for t in tables]
        ns = (C.c_size_t * max(k, 1))(*[len(t) for t in tables])
        ptrs = (u64p * max(k, 1))(*[p for _, p in arrs])
        outs = [_out_u64(len(t)) for t in tables]
        optrs = (u64p * max(k, 1))(*[p for _, p in outs])
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_product_layers_batch(self.h, k, ptrs, ns, optrs, C.byref(bad)), bad)
        return [o[:len(t)] for (o, _), t in zip(outs, tables)]

    def dev_product_layers_batch(self, d_tables, ns, d_out):
        """zigz_dev_product_layers_batch: device columns (packed u32 canonical, 16-byte aligned; only read) into device buffers of
        ns[i] u32 words each (addresses, 16-byte aligned): queued on the context's stream, not waited for."""
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        ptrs = (vp * max(k, 1))(*[int(d) for d in d_tables])
        optrs = (vp * max(k, 1))(*[int(d) for d in d_out])
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_dev_product_layers_batch(self.h, k, ptrs, nsa, optrs, C.byref(bad)), bad)

    def _grand_product_prove(self, fn, ptrs, ns, challenges):
        k = len(ns)
        vs = [max(int(n).bit_length() - 1, 0) for n in ns]
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        pr, prp = _out_u64(k)
        ev, evp = _out_u64(sum(2 * v for v in vs))
        r, rp = _out_u64(sum(2 * v * (v - 1) for v in vs))
        pt, ptp = _out_u64(sum(v * (v - 1) // 2 for v in vs))
        lc, lcp = _out_u64(sum(vs))
        lp, lpp = _out_u64(sum(vs))
        le, lep = _out_u64(k)
        cp = None
        if challenges is not None:
            c, cp = self._cat_u64(challenges)
        bad = C.c_size_t(0)
        self.check_batch(fn(self.h, k, ptrs, nsa, cp, prp, evp, rp, ptp, lcp, lpp, lep, C.byref(bad)), bad)
        out, eo, ro, po, vo = [], 0, 0, 0, 0
        for i, v in enumerate(vs):
            out.append((int(pr[i]), ev[eo: eo + 2 * v].copy(), r[ro: ro + 2 * v * (v - 1)].copy(), pt[po: po + v * (v - 1) // 2].copy(),
                        lc[vo: vo + v].copy(), lp[vo: vo + v].copy(), int(le[i])))
            eo, ro, po, vo = eo + 2 * v, ro + 2 * v * (v - 1), po + v * (v - 1) // 2, vo + v
        return out

    def grand_product_prove_batch(self, tables, challenges=None):
        """zigz_grand_product_prove_batch: for every column (2^v canonical words) the layered grand-product proof (product,
        layer_evals [2 v], rounds [2 v (v - 1)], points [v (v - 1) / 2], layer_challenges [v], leaf_point [v], leaf_eval);
        challenges[i] (optional, v (v + 1) / 2 words in order of use) fixes instance i's challenges (no transcript)."""
        arrs = [_u64(t) for t in tables]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        return self._grand_product_prove(lib.zigz_grand_product_prove_batch, ptrs, [len(t) for t in tables], challenges)

    def dev_grand_product_prove_batch(self, d_tables, ns, challenges=None):
        """zigz_dev_grand_product_prove_batch over device-resident columns (packed u32 canonical, 16-byte aligned; only read)."""
        ptrs = (vp * max(len(ns), 1))(*[int(d) for d in d_tables])
        return self._grand_product_prove(lib.zigz_dev_grand_product_prove_batch, ptrs, ns, challenges)

    def _grand_product_verify(self, fn, ptrs, ns, proofs, flags):
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        pr, prp = self._cat_u64([[int(p[0]) for p in proofs]])
        ev, evp = self._cat_u64([p[1] for p in proofs])
        r, rp = self._cat_u64([p[2] for p in proofs])
        lp, lpp = self._cat_u64([p[5] for p in proofs])
        le, lep = self._cat_u64([[int(p[6]) for p in proofs]])
        verd, vdp = _out_u8(k)
        exp, ep = _out_u64(k)
        orc, op = _out_u64(k)
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        self.check_batch(fn(self.h, k, ptrs, nsa, prp, evp, rp, lpp, lep, int(flags), vdp, ep, op, C.byref(rej), C.byref(bad)), bad)
        deferred = bool(int(flags) & GRAND_PRODUCT_LEAF_DEFERRED)
        return verd[:k].copy(), [int(x) for x in exp[:k]], [None if deferred else int(x) for x in orc[:k]], rej.value

    def grand_product_verify_batch(self, tables, proofs, flags=0, ns=None):
        """zigz_grand_product_verify_batch: proofs[i] as grand_product_prove_batch returns it (Fiat-Shamir), tables[i] the column.
        flags = GRAND_PRODUCT_LEAF_DEFERRED: tables must be None and ns gives the lengths; the column's evaluation at the leaf
        point is then the caller's check.  Returns (verdicts np.uint8, expected_evals, oracle_evals, n_rejected)."""
        if tables is None:
            return self._grand_product_verify(lib.zigz_grand_product_verify_batch, None, ns, proofs, flags)
        arrs = [_u64(t) for t in tables]
        ptrs = (u64p * max(len(arrs), 1))(*[p for _, p in arrs])
        return self._grand_product_verify(lib.zigz_grand_product_verify_batch, ptrs, [len(t) for t in tables], proofs, flags)

    def dev_grand_product_verify_batch(self, d_tables, ns, proofs, flags=0):
        """zigz_dev_grand_product_verify_batch over device-resident columns (d_tables None with GRAND_PRODUCT_LEAF_DEFERRED)."""
        ptrs = None if d_tables is None else (vp * max(len(ns), 1))(*[int(d) for d in d_tables])
        return self._grand_product_verify(lib.zigz_dev_grand_product_verify_batch, ptrs, ns, proofs, flags)

    def _merkle_batch_out(self, rc, bad, k, roots, heights, handle, ns, keep):
        self.check_batch(rc, bad)
        res = [(roots[32 * i: 32 * (i + 1)].tobytes(), int(heights[i])) for i in range(k)]
        return res, (MerkleBatch(self, handle, ns, [h for _, h in res]) if keep and k else None)

    def merkle_commit_batch(self, tables, keep=True):
        """zigz_merkle_commit_batch: SimpleMerkleTree.build(t) for every table (any lengths), in shared launches
        (CommitmentScheme.batchCommit).  Returns ([(root, height)], MerkleBatch or None when keep is False)."""
        k = len(tables)
        arrs = [_u64(t) for t in tables]
        ns = (C.c_size_t * max(k, 1))(*[len(t) for t in tables])
        ptrs = (u64p * max(k, 1))(*[p for _, p in arrs])
        roots, rp = _out_u8(32 * k)
        heights = (C.c_size_t * max(k, 1))()
        h, bad = vp(), C.c_size_t(0)
        rc = lib.zigz_merkle_commit_batch(self.h, ptrs, ns, k, rp, heights, C.byref(h) if keep else None, C.byref(bad))
        return self._merkle_batch_out(rc, bad, k, roots, heights, h, [len(t) for t in tables], keep)

    def dev_merkle_commit_batch(self, d_tables, ns, keep=True):
        """zigz_dev_merkle_commit_batch over device-resident tables (packed u32 canonical, 4-byte aligned)."""
        k = len(ns)
        nsa = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        ptrs = (vp * max(k, 1))(*[int(d) for d in d_tables])
        roots, rp = _out_u8(32 * k)
        heights = (C.c_size_t * max(k, 1))()
        h, bad = vp(), C.c_size_t(0)
        rc = lib.zigz_dev_merkle_commit_batch(self.h, ptrs, nsa, k, rp, heights, C.byref(h) if keep else None, C.byref(bad))
        return self._merkle_batch_out(rc, bad, k, roots, heights, h, [int(n) for n in ns], keep)

    def commit_open_batch(self, batch, points):
        """zigz_commit_open_batch: CommitmentScheme.open(poly_i, tree_i, points[i]) for every table of the batch (each table
        2^v values, points[i] of v coordinates).  Returns per-table dicts like CommitmentScheme.open."""
        k, tot = len(batch.heights), sum(batch.heights)
        if len(points) != k or any(len(p) != h for p, h in zip(points, batch.heights)):
            raise ValueError("points[i] must have heights[i] coordinates, one point per table")
        q, qp = _u64(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in points] + [np.zeros(1, np.uint64)]))
        vals, vlp = _out_u64(k)
        idx, ip = _out_u64(k)
        leaf, lp = _out_u64(k)
        sib, sp = _out_u8(32 * tot)
        dirs, dp = _out_u8(tot)
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_commit_open_batch(self.h, batch.h, qp, vlp, ip, sp, dp, lp, C.byref(bad)), bad)
        out, o = [], 0
        for i, v in enumerate(batch.heights):
            out.append(dict(value=int(vals[i]), index=int(idx[i]), leaf=int(leaf[i]), siblings=sib[32 * o: 32 * (o + v)].tobytes(),
                            directions=dirs[o: o + v].tobytes()))
            o += v
        return out

    # ---- batched Merkle verification (one lane per opening)
    def _verify_batch(self, fn, k, roots, heights, leaves, siblings, dirs):
        hs = (C.c_size_t * max(k, 1))(*[int(h) for h in heights])
        verd, vp_ = _out_u8(k)
        rej, bad = C.c_size_t(0), C.c_size_t(0)
        self.check_batch(fn(self.h, k, roots, hs, leaves, siblings, dirs, vp_, C.byref(rej), C.byref(bad)), bad)
        return verd[:k].copy()

    def merkle_verify_batch(self, roots, heights, leaves, siblings, dirs):
        """zigz_merkle_verify_batch: SimpleMerkleTree.verify for k openings -- roots (k x 32 bytes), heights, leaf values (u64,
        hashed as given), siblings (32 B each) and directions packed opening by opening.  Returns the np.uint8 verdicts."""
        k = len(heights)
        r = np.frombuffer(bytes(roots) + b"\0" * 32, dtype=np.uint8).copy()
        if len(r) != 32 * k + 32:
            raise ValueError(f"{len(r) - 32} root bytes for {k} openings")
        lv, lp = _u64(np.asarray(leaves, dtype=np.uint64).reshape(-1))
        sib = np.frombuffer(bytes(siblings) + b"\0" * 32, dtype=np.uint8).copy()
        d = np.frombuffer(bytes(dirs) + b"\0", dtype=np.uint8).copy()
        tot = sum(int(h) for h in heights)
        if len(lv) < k or len(sib) != 32 * tot + 32 or len(d) != tot + 1:
            raise ValueError("leaves, siblings and dirs must hold k values, 32 * sum(heights) and sum(heights) bytes")
        return self._verify_batch(lib.zigz_merkle_verify_batch, k, r.ctypes.data_as(u8p), heights, lp, sib.ctypes.data_as(u8p),
                                  d.ctypes.data_as(u8p))

    def dev_merkle_verify_batch(self, d_roots, heights, d_leaves, d_siblings, d_dirs):
        """zigz_dev_merkle_verify_batch over device-resident roots (16-byte aligned), leaf values (u64, 8-byte aligned),
        siblings (16-byte aligned) and directions in the layout of merkle_verify_batch; heights on the host."""
        return self._verify_batch(lib.zigz_dev_merkle_verify_batch, len(heights), vp(d_roots), heights, vp(d_leaves),
                                  vp(d_siblings), vp(d_dirs))

    def commit_verify_batch(self, commitments, proofs):
        """CommitmentScheme.batchVerify (polynomial_commit.zig:160-175) on the device, over the input of host.batch_verify:
        (root, num_vars) pairs and dicts with point, value, index, leaf, siblings and directions.  Returns (all_ok, verdicts).
        verify's rule per opening (:123-125): a point of another length than num_vars rejects that opening alone; the index and
        value are not checked.  A path whose directions and siblings differ in number, or higher than any tree (64), is
        rejected too.  len(commitments) != len(proofs): (False, None), like batchVerify (:164-166)."""
        k = len(commitments)
        if k != len(proofs):
            return False, None
        verd = np.zeros(k, dtype=np.uint8)
        sel = [i for i, ((_, v), p) in enumerate(zip(commitments, proofs))
               if len(p["point"]) == v and len(p["siblings"]) == 32 * len(p["directions"]) and len(p["directions"]) <= 64]
        if sel:
            got = self.merkle_verify_batch(b"".join(bytes(commitments[i][0]) for i in sel), [len(proofs[i]["directions"]) for i in sel],
                                           [int(proofs[i]["leaf"]) for i in sel], b"".join(bytes(proofs[i]["siblings"]) for i in sel),
                                           b"".join(bytes(proofs[i]["directions"]) for i in sel))
            verd[sel] = got
        return bool(verd.all()), verd

    def lasso_prove_batch(self, instances):
        """zigz_lasso_prove_batch: instances are dicts with table, queries and optional n_in (2), n_out (1), mapping (None).
        Returns the list of lasso_prove() dicts."""
        k = len(instances)
        n = max(k, 1)
        keep = []
        tabs, qs, maps, routs, pouts = (u64p * n)(), (u64p * n)(), (u64p * n)(), (u64p * n)(), (u64p * n)()
        rows, nqs, nins, nouts, nmaps = [(C.c_size_t * n)() for _ in range(5)]
        outs = []
        for i, d in enumerate(instances):
            n_in, n_out = d.get("n_in", 2), d.get("n_out", 1)
            w = n_in + n_out
            t, tabs[i] = _u64(np.asarray(d["table"], dtype=np.uint64).reshape(-1))
            q, qs[i] = _u64(np.asarray(d["queries"], dtype=np.uint64).reshape(-1))
            rows[i] = 0 if len(d["table"]) == 0 or w == 0 else len(np.asarray(d["table"]).reshape(-1)) // w
            nqs[i] = nq = len(d["queries"])
            nins[i], nouts[i] = n_in, n_out
            npad = 1
            while npad < max(nq, 1):
                npad <<= 1
            nvmax = npad.bit_length() - 1
            r, routs[i] = _out_u64(2 * nvmax)
            pt, pouts[i] = _out_u64(nvmax)
            keep += [t, q]
            if d.get("mapping") is not None:
                m, maps[i] = _u64(d["mapping"])
                nmaps[i] = len(d["mapping"])
                keep.append(m)
            outs.append((r, pt))
        nv = (C.c_size_t * n)()
        fe, fep = _out_u64(n)
        qc, qcp = _out_u8(32 * n)
        tc, tcp = _out_u8(32 * n)
        bad = C.c_size_t(0)
        self.check_batch(lib.zigz_lasso_prove_batch(self.h, k, tabs, rows, qs, nqs, nins, nouts, maps, nmaps, nv, routs, pouts, fep,
                                                    qcp, tcp, C.byref(bad)), bad)
        out = []
        for i, (r, pt) in enumerate(outs):
            v = nv[i]
            out.append(dict(nv=v, rounds=r[: 2 * v].copy(), point=pt[:v].copy(), final_eval=int(fe[i]),
                            query_commit=qc[32 * i: 32 * i + 32].tobytes(), table_commit=tc[32 * i: 32 * i + 32].tobytes()))
        return out

    # ---- Lasso
    def lasso_fingerprints(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n, w = rows.shape
        o, op = _out_u64(n)
        self.check(lib.zigz_lasso_fingerprints(self.h, rows.ctypes.data_as(u64p), n, w, op))
        return o[:n]

    def lasso_prove(self, table, queries, n_in=2, n_out=1, mapping=None):
        """LassoProver.prove / proveWithMapping, lasso_prover.zig:103,179"""
        w = n_in + n_out
        t, tp = _u64(np.asarray(table, dtype=np.uint64).reshape(-1))
        q, qp = _u64(np.asarray(queries, dtype=np.uint64).reshape(-1))
        rows = 0 if len(table) == 0 else len(np.asarray(table).reshape(-1)) // w
        nq = len(queries)
        npad = 1
        while npad < max(nq, 1):
            npad <<= 1
        nvmax = npad.bit_length() - 1
        r, rp = _out_u64(2 * nvmax)
        pt, ptp = _out_u64(nvmax)
        fe = C.c_uint64()
        nv = C.c_size_t()
        qc, qcp = _out_u8(32)
        tc, tcp = _out_u8(32)
        if mapping is None:
            self.check(lib.zigz_lasso_prove(self.h, tp, rows, qp, nq, n_in, n_out, C.byref(nv), rp, ptp, C.byref(fe),
                                            qcp, tcp))
        else:
            m, mp = _u64(mapping)
            self.check(lib.zigz_lasso_prove_with_mapping(self.h, tp, rows, qp, nq, n_in, n_out, mp, len(mapping),
                                                         C.byref(nv), rp, ptp, C.byref(fe), qcp, tcp))
        v = nv.value
        return dict(nv=v, rounds=r[: 2 * v].copy(), point=pt[:v].copy(), final_eval=fe.value,
                    query_commit=qc.tobytes(), table_commit=tc.tobytes())


class SimpleMerkleTree:
    """SimpleMerkleTree(F, SHA3Hasher), merkle_tree.zig:273 -- all levels resident in HBM."""

    def __init__(self, ctx, values):
        self.ctx = ctx
        a, ap = _u64(values)
        root, rp = _out_u8(32)
        h = C.c_size_t()
        t = vp()
        ctx.check(lib.zigz_merkle_commit(ctx.h, ap, len(values), rp, C.byref(h), C.byref(t)))
        self.root_hash = root.tobytes()
        self.height = h.value
        self.n_values = len(values)
        self.t = t

    @classmethod
    def build(cls, ctx, values):
        return cls(ctx, values)

    def getRoot(self):
        return self.root_hash

    def open(self, index):
        sib, sp = _out_u8(32 * self.height)
        dirs, dp = _out_u8(self.height)
        leaf = C.c_uint64()
        self.ctx.check(lib.zigz_merkle_open(self.ctx.h, self.t, index, sp, dp, C.byref(leaf)))
        return dict(index=index, value=leaf.value, siblings=sib[: 32 * self.height].tobytes(),
                    directions=dirs[: self.height].tobytes())

    def deinit(self):
        if self.t:
            lib.zigz_merkle_destroy(self.ctx.h, self.t)
            self.t = None

    def __del__(self):
        try:
            self.deinit()
        except Exception:
            pass


class MerkleBatch:
    """The trees of one zigz_merkle_commit_batch call (Context.merkle_commit_batch): values and trees of all tables in one
    device allocation."""

    def __init__(self, ctx, h, ns, heights):
        self.ctx, self.h, self.ns, self.heights = ctx, h, list(ns), list(heights)

    def open(self, indices):
        """zigz_merkle_open_batch: tree_i.open(indices[i]) for every tree; per-tree dicts like SimpleMerkleTree.open"""
        k, tot = len(self.heights), sum(self.heights)
        ix, ixp = _u64(np.asarray(indices, dtype=np.uint64).reshape(-1))
        if len(indices) != k:
            raise ValueError(f"{len(indices)} indices for {k} trees")
        leaf, lp = _out_u64(k)
        sib, sp = _out_u8(32 * tot)
        dirs, dp = _out_u8(tot)
        bad = C.c_size_t(0)
        self.ctx.check_batch(lib.zigz_merkle_open_batch(self.ctx.h, self.h, ixp, sp, dp, lp, C.byref(bad)), bad)
        out, o = [], 0
        for i, v in enumerate(self.heights):
            out.append(dict(index=int(ix[i]), value=int(leaf[i]), siblings=sib[32 * o: 32 * (o + v)].tobytes(),
                            directions=dirs[o: o + v].tobytes()))
            o += v
        return out

    def _many_args(self, trees, indices):
        t = np.ascontiguousarray(np.asarray(trees, dtype=np.uint32).reshape(-1))
        ix = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(-1))
        if len(t) != len(ix):
            raise ValueError(f"{len(t)} trees for {len(ix)} indices")
        hs = np.asarray(self.heights + [0], dtype=np.int64)[np.minimum(t, len(self.heights))]  # (a bad tree id: the call rejects it)
        pad = (lambda a: a if a.size else np.zeros(1, a.dtype))
        return pad(t), pad(ix), len(t), int(hs.sum())

    def open_many(self, trees, indices):
        """zigz_merkle_open_many: tree_{trees[j]}.open(indices[j]) for every j, any number per tree.  Returns a dict of numpy
        arrays in the shapes Context.merkle_verify_batch takes: roots (k x 32), heights (k), leaves (k), and siblings (32 B
        each) and dirs packed opening by opening."""
        t, ix, k, tot = self._many_args(trees, indices)
        sib, sp = _out_u8(32 * tot)
        dirs, dp = _out_u8(tot)
        leaf, lp = _out_u64(k)
        roots, rp = _out_u8(32 * k)
        hs = (C.c_size_t * max(k, 1))()
        bad = C.c_size_t(0)
        self.ctx.check_batch(lib.zigz_merkle_open_many(self.ctx.h, self.h, k, t.ctypes.data_as(u32p), ix.ctypes.data_as(u64p), sp, dp,
                                                       lp, rp, hs, C.byref(bad)), bad)
        return dict(roots=roots[: 32 * k].reshape(k, 32), heights=np.array(hs[:k], dtype=np.int64), leaves=leaf[:k],
                    siblings=sib[: 32 * tot], dirs=dirs[:tot])

    def dev_open_many(self, trees, indices, d_siblings, d_dirs, d_leaves, d_roots=None):
        """zigz_dev_merkle_open_many: the same into device memory (addresses; d_siblings and d_roots 16-byte aligned, d_leaves
        8-byte aligned) in the layout Context.dev_merkle_verify_batch takes; queued on the context's stream.  Returns the
        heights (host)."""
        t, ix, k, _ = self._many_args(trees, indices)
        hs = (C.c_size_t * max(k, 1))()
        bad = C.c_size_t(0)
        self.ctx.check_batch(lib.zigz_dev_merkle_open_many(self.ctx.h, self.h, k, t.ctypes.data_as(u32p), ix.ctypes.data_as(u64p),
                                                           vp(d_siblings), vp(d_dirs), vp(d_leaves), vp(d_roots) if d_roots else None,
                                                           hs, C.byref(bad)), bad)
        return np.array(hs[:k], dtype=np.int64)

    def deinit(self):
        if self.h:
            lib.zigz_merkle_batch_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.deinit()
        except Exception:
            pass


class CommitmentScheme:
    """CommitmentSchemeSHA3(F), polynomial_commit.zig:58-185"""

    @staticmethod
    def commit(ctx, evals):
        tree = SimpleMerkleTree(ctx, evals)
        return tree.root_hash, tree

    @staticmethod
    def open(ctx, evals, tree, point):
        nv = len(point)
        a, ap = (None, None) if evals is None else _u64(evals)
        n = tree.n_values if evals is None else len(evals)
        q, qp = _u64(point)
        sib, sp = _out_u8(32 * nv)
        dirs, dp = _out_u8(nv)
        val, idx, leaf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ctx.check(lib.zigz_commit_open(ctx.h, ap, n, tree.t, qp, nv, C.byref(val), C.byref(idx), sp, dp, C.byref(leaf)))
        return dict(value=val.value, index=idx.value, leaf=leaf.value, siblings=sib[: 32 * nv].tobytes(),
                    directions=dirs[:nv].tobytes())


class CommitJob:
    """Prover.generateCommitments split at its transcript dependencies (prover.zig:366-467)."""

    def __init__(self, ctx, cols=None, d_cols=None, ncols=NUM_COLUMNS, nv=None, col_stride=None, d_cols_list=None):
        self.ctx = ctx
        j = vp()
        if d_cols_list is not None:  # zigz_commit_begin_batch: several proofs' resident columns in one job
            k = len(d_cols_list)
            arr = (vp * k)(*[vp(d) for d in d_cols_list])
            ctx.check(lib.zigz_commit_begin_batch(ctx.h, arr, k, ncols, col_stride or (1 << nv), nv, C.byref(j)))
            ncols = ncols * k
        elif cols is not None:
            cols = np.ascontiguousarray(cols, dtype=np.uint64)
            ncols, N = cols.shape
            nv = N.bit_length() - 1
            self._keep = cols
            ctx.check(lib.zigz_commit_begin(ctx.h, cols.ctypes.data_as(u64p), ncols, N, nv, C.byref(j)))
        else:
            ctx.check(lib.zigz_commit_begin_dev(ctx.h, vp(d_cols), ncols, col_stride or (1 << nv), nv, C.byref(j)))
        self.j, self.ncols, self.nv = j, ncols, nv

    def roots(self):
        r, rp = _out_u8(self.ncols * 32)
        self.ctx.check(lib.zigz_commit_roots(self.j, rp))
        return r[: self.ncols * 32].reshape(self.ncols, 32)

    def open_all(self, points):
        nc, nv = self.ncols, self.nv
        p, pp = _u64(np.asarray(points, dtype=np.uint64).reshape(-1))
        values, vpp = _out_u64(nc)
        idx, ip = _out_u64(nc)
        leaves, lp = _out_u64(nc)
        sib, sp = _out_u8(nc * nv * 32)
        dirs, dp = _out_u8(nc * nv)
        self.ctx.check(lib.zigz_commit_open_all(self.j, pp, vpp, ip, lp, sp, dp))
        return dict(values=values[:nc], indices=idx[:nc], leaves=leaves[:nc],
                    siblings=sib[: nc * nv * 32].reshape(nc, nv, 32), dirs=dirs[: nc * nv].reshape(nc, nv))

    def open_many(self, cols, indices):
        """zigz_commit_open_many: k openings of the job's trees (cols[j] in the job's column numbering, indices[j] < 2^nv),
        valid after roots().  Returns dict(leaves (k), siblings (k x nv x 32), dirs (k x nv))."""
        if not self.j:  # ended: the handle is gone
            raise errors.ZigzError(errors.BAD_STATE, _name(errors.BAD_STATE), "the commit job has ended")
        c = np.ascontiguousarray(np.asarray(cols, dtype=np.uint32).reshape(-1))
        ix = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(-1))
        if len(c) != len(ix):
            raise ValueError(f"{len(c)} columns for {len(ix)} indices")
        k, nv = len(c), self.nv
        if k == 0:
            c, ix = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        sib, sp = _out_u8(k * nv * 32)
        dirs, dp = _out_u8(k * nv)
        leaf, lp = _out_u64(k)
        bad = C.c_size_t(0)
        self.ctx.check_batch(lib.zigz_commit_open_many(self.j, k, c.ctypes.data_as(u32p), ix.ctypes.data_as(u64p), sp, dp, lp,
                                                       C.byref(bad)), bad)
        return dict(leaves=leaf[:k], siblings=sib[: k * nv * 32].reshape(k, nv, 32), dirs=dirs[: k * nv].reshape(k, nv))

    def tree(self):
        """(device address, bytes per column) of the built trees, internal node form -- for node-by-node comparisons."""
        d, n = vp(), C.c_size_t()
        self.ctx.check(lib.zigz_commit_job_tree(self.j, C.byref(d), C.byref(n)))
        return d.value, n.value

    def end(self):
        if self.j:
            lib.zigz_commit_end(self.j)
            self.j = None

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


class Transcript:
    """FiatShamirTranscript (src/core/hash.zig:255-324), BabyBear challenges."""

    def __init__(self):
        self.h = lib.zigz_transcript_new()

    def __del__(self):
        if getattr(self, "h", None):
            lib.zigz_transcript_free(self.h)
            self.h = None

    def append_bytes(self, b):
        lib.zigz_transcript_append_bytes(self.h, bytes(b), len(b))

    def append_field(self, v):
        lib.zigz_transcript_append_field(self.h, int(v))

    def append_tagged_counter(self, tag, start, count):
        lib.zigz_transcript_append_tagged_counter(self.h, bytes(tag), len(tag), start, count)

    def challenge(self):
        return lib.zigz_transcript_challenge(self.h)


def sha3_256(b):
    o, op = _out_u8(32)
    lib.zigz_sha3_256(bytes(b), len(b), op)
    return o.tobytes()


def sha256(b):
    o, op = _out_u8(32)
    lib.zigz_sha256(bytes(b), len(b), op)
    return o.tobytes()
