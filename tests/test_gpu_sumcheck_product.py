"""The batched product sumcheck prover on the GPU (zigz_dev_sumcheck_prove_product_batch, zigz_sumcheck_prove_product_batch): every
output word of every instance equals the numpy reference (sumcheck_product_ref.py) -- on both sides of the host-tail threshold
(1024) and of a workgroup's chunk (8192), for d = 1..3, with Fiat-Shamir and fixed challenges; d = 1 is bytes-equal to the linear
batched prover; a batch equals its instances proved alone and needs nothing zeroed between calls; the caller's tables may repeat
and are never written; the exact sums do not wrap at 2^20 with every term maximal; errors touch nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sumcheck_product_ref as R

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
TAIL = 1024   # HOST_TAIL_MAX: tables this long finish on the host
CHUNK = 8192  # PRODUCT_CHUNK (kernels.hpp): elements of the current table per workgroup
SIZES = [2, 4, 16, TAIL, 2 * TAIL, 4096, CHUNK, 2 * CHUNK, 4 * CHUNK]


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


class DevTables:
    """tables uploaded into one device buffer, each 16-byte aligned (offsets in u32 words: multiples of 4)"""

    def __init__(self, ctx, tables):
        self.ctx, self.tables = ctx, tables
        self.off, o = [], 0
        for t in tables:
            self.off.append(o)
            o += (len(t) + 3) // 4 * 4
        packed = np.zeros(max(o, 4), dtype=np.uint64)
        for t, a in zip(tables, self.off):
            packed[a:a + len(t)] = t
        self.words = len(packed)
        self.packed = packed
        self.base = ctx.dev_alloc(len(packed) * 4)
        ctx.upload(packed, self.base)
        self.ptrs = [self.base + 4 * a for a in self.off]

    def unchanged(self):
        return np.array_equal(self.ctx.download(self.base, self.words), self.packed)

    def free(self):
        self.ctx.dev_free(self.base)


def _tables(seed, d, n):
    return [O.splitmix64_field(seed + 17 * j, n) for j in range(d)]


@pytest.fixture(scope="module")
def singles(ctx):
    """per size three tables on the device, and per (size, degree) the reference's Fiat-Shamir and fixed-challenge proofs of the
    first d of them (computed once)"""
    out = {}
    for n in SIZES:
        fs = _tables(51000 + n, 3, n)
        ch = O.splitmix64_field(52000 + n, n.bit_length() - 1)
        out[n] = (fs, ch, {d: (R.prove(fs[:d]), R.prove(fs[:d], ch)) for d in (1, 2, 3)})
    dev = DevTables(ctx, [t for n in SIZES for t in out[n][0]])
    yield out, {n: dev.ptrs[3 * i: 3 * i + 3] for i, n in enumerate(SIZES)}
    dev.free()


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_single_instances(ctx, singles, n, d):
    ref, ptrs = singles
    fs, ch, proofs = ref[n]
    fiat, fixed = proofs[d]
    got = ctx.dev_sumcheck_prove_product_batch([ptrs[n][:d]], [n])
    assert len(got) == 1 and R.same(got[0], fiat), (n, d, "fiat-shamir")
    got = ctx.dev_sumcheck_prove_product_batch([ptrs[n][:d]], [n], [ch])
    assert R.same(got[0], fixed), (n, d, "fixed")
    if n == 4 * CHUNK:  # the reference itself: a verifier with oracle access accepts it
        R.check_proof(fs[:d], got[0], fiat_shamir=False)


@pytest.mark.parametrize("n", [1 << 12, 1 << 16])
def test_degree_one_is_the_linear_prover(ctx, n):
    t = O.splitmix64_field(53000 + n, n)
    ch = O.splitmix64_field(53100 + n, n.bit_length() - 1)
    dev = DevTables(ctx, [t])
    try:
        for c in (None, [ch]):
            (rounds, point, fe), = ctx.dev_sumcheck_prove_batch(dev.ptrs, [n], c)
            (claimed, r2, p2, evals, fe2), = ctx.dev_sumcheck_prove_product_batch([dev.ptrs], [n], c)
            assert rounds.tobytes() == r2.tobytes() and point.tobytes() == p2.tobytes() and fe == fe2 == int(evals[0])
            assert claimed == O.mle_sum(P, t)
    finally:
        dev.free()


def test_mixed_batch_equals_its_instances_alone(ctx):
    logs = [9, 16, 1, 13, 11, 5, 14]  # not sorted by size; both sides of the tail threshold and of a chunk
    degs = [2, 3, 1, 3, 2, 3, 1]
    inst = [_tables(54000 + 100 * i, d, 1 << v) for i, (v, d) in enumerate(zip(logs, degs))]
    ns = [1 << v for v in logs]
    dev = DevTables(ctx, [t for fs in inst for t in fs])
    try:
        ptrs, o = [], 0
        for d in degs:
            ptrs.append(dev.ptrs[o: o + d])
            o += d
        batch = ctx.dev_sumcheck_prove_product_batch(ptrs, ns)
        for i in range(7):
            alone, = ctx.dev_sumcheck_prove_product_batch([ptrs[i]], [ns[i]])
            assert R.same(batch[i], alone), i
            assert R.same(batch[i], R.prove(inst[i])), i
        # again on the same context, and a different batch in between: nothing needed zeroing
        other = ctx.dev_sumcheck_prove_product_batch(ptrs[::-1], ns[::-1])
        again = ctx.dev_sumcheck_prove_product_batch(ptrs, ns)
        for i in range(7):
            assert R.same(again[i], batch[i]) and R.same(other[6 - i], batch[i]), i
        assert dev.unchanged()
    finally:
        dev.free()


def test_one_table_as_several_factors_and_in_several_instances(ctx):
    n = 1 << 13
    f, g = O.splitmix64_field(55000, n), O.splitmix64_field(55001, n)
    dev = DevTables(ctx, [f, g])
    try:
        pf, pg = dev.ptrs
        got = ctx.dev_sumcheck_prove_product_batch([[pf, pf], [pf, pf, pg], [pg, pf], [pf]], [n] * 4)
        for proof, fs in zip(got, ([f, f], [f, f, g], [g, f], [f])):
            assert R.same(proof, R.prove(fs))
        assert dev.unchanged()  # the caller's tables are read only
    finally:
        dev.free()


def test_sums_do_not_wrap_at_2p20(ctx):
    """every coefficient term maximal: all p - 1 (d = 3), and low half 0 / high half p - 1 (d = 2: a = 0, b - a = p - 1)"""
    n = 1 << 20
    top = np.full(n, P - 1, dtype=np.uint64)
    step = np.concatenate([np.zeros(n // 2, dtype=np.uint64), np.full(n // 2, P - 1, dtype=np.uint64)])
    dev = DevTables(ctx, [top, step])
    try:
        got = ctx.dev_sumcheck_prove_product_batch([[dev.ptrs[0]] * 3, [dev.ptrs[1]] * 2], [n, n])
        assert R.same(got[0], R.prove([top] * 3))
        assert R.same(got[1], R.prove([step] * 2))
        assert got[0][0] == (P - n % P) % P  # (-1)^3 summed n times
    finally:
        dev.free()


def _raw(ctx, fn, ptr_t, ptrs, degs, ns):
    """the raw entry over prefilled output buffers: (status, bad_index, outputs untouched)"""
    from zigz_amd._ffi import u64p
    k = len(ns)
    outs = [np.full(64 * k + 64, 0xABCDEF, dtype=np.uint64) for _ in range(5)]
    bad = C.c_size_t(12345)
    rc = fn(ctx.h, k, (C.c_uint * k)(*degs), (ptr_t * len(ptrs))(*ptrs), (C.c_size_t * k)(*ns), None,
            *[o.ctypes.data_as(u64p) for o in outs], C.byref(bad))
    return rc, bad.value, all(np.all(o == 0xABCDEF) for o in outs)


def test_host_form_equals_device_form(ctx):
    from zigz_amd._ffi import lib, u64p
    ns = [1 << 12, 1 << 6, 1 << 14]
    degs = [3, 2, 2]
    inst = [_tables(56000 + 100 * i, d, n) for i, (n, d) in enumerate(zip(ns, degs))]
    ch = [O.splitmix64_field(56500 + i, n.bit_length() - 1) for i, n in enumerate(ns)]
    dev = DevTables(ctx, [t for fs in inst for t in fs])
    try:
        ptrs = [dev.ptrs[0:3], dev.ptrs[3:5], dev.ptrs[5:7]]
        for c in (None, ch):
            host = ctx.sumcheck_prove_product_batch(inst, c)
            devf = ctx.dev_sumcheck_prove_product_batch(ptrs, ns, c)
            for i in range(3):
                assert R.same(host[i], devf[i]) and R.same(host[i], R.prove(inst[i], None if c is None else c[i])), i
    finally:
        dev.free()
    assert ctx.sumcheck_prove_product_batch([]) == []
    # a value >= p in instance 1: its index, and nothing written
    bad = [[t.copy() for t in fs] for fs in inst]
    bad[1][1][5] = P
    arrs = [np.ascontiguousarray(t) for fs in bad for t in fs]
    rc, idx, untouched = _raw(ctx, lib.zigz_sumcheck_prove_product_batch, u64p, [a.ctypes.data_as(u64p) for a in arrs], degs, ns)
    assert (rc, idx, untouched) == (E.NOT_CANONICAL, 1, True)
    with pytest.raises(E.ZigzError) as e:
        ctx.sumcheck_prove_product_batch(bad)
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1


def test_errors_name_the_first_failing_instance_and_touch_nothing(ctx):
    from zigz_amd._ffi import lib, vp
    n = 1 << 11
    dev = DevTables(ctx, _tables(57000, 3, n))
    try:
        p = dev.ptrs
        fn = lib.zigz_dev_sumcheck_prove_product_batch
        assert _raw(ctx, fn, vp, [p[0], p[1], p[2]], [1, 2], [n, n]) == (0, 12345, False)
        for ptrs, degs, ns, code, idx in [([p[0], p[1] + 4, p[2]], [1, 2], [n, n], E.INVALID_ARGUMENT, 1),
                                          ([p[0], p[1], 0], [1, 2], [n, n], E.INVALID_ARGUMENT, 1),
                                          ([p[0], p[1], p[2], p[2]], [4, 1], [n, n], E.INVALID_ARGUMENT, 0),
                                          ([p[0], p[1]], [1, 0], [n, n], E.INVALID_ARGUMENT, 1),
                                          ([p[0], p[1], p[2]], [2, 1], [n, 1], E.NO_VARIABLES, 1),
                                          ([p[0], p[1], p[2]], [2, 1], [n, 24], E.LENGTH_NOT_POWER_OF_TWO, 1),
                                          ([p[0], p[1], p[2]], [1, 2], [n, 1 << 31], E.INVALID_ARGUMENT, 1)]:
            assert _raw(ctx, fn, vp, ptrs, degs, ns) == (code, idx, True), (degs, ns)
        assert _raw(ctx, fn, vp, [p[0]] * 4097, [1] * 4097, [n] * 4097)[0] == E.INVALID_ARGUMENT
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_sumcheck_prove_product_batch([[p[0]], [p[1], p[2]]], [n, n], [np.zeros(11, np.uint64), np.full(11, P, np.uint64)])
        assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    finally:
        dev.free()


def test_inside_an_active_commit_job(ctx):
    import zigz_amd
    nv = 11
    cols = np.stack([O.splitmix64_field(58000 + c, 1 << nv) for c in range(43)])
    cexp = O.generate_commitments(P, O.Transcript(), cols, fast=True)
    ns = [1 << 13, 1 << 4, 1 << 11]
    degs = [3, 2, 1]
    inst = [_tables(58100 + 100 * i, d, n) for i, (n, d) in enumerate(zip(ns, degs))]
    ref = [R.prove(fs) for fs in inst]
    dev = DevTables(ctx, [t for fs in inst for t in fs])
    opts = ("run_aware_mask", "cons_group_mask", "small_domain_mask", "per_round_sumcheck", "fold_eval")
    job = zigz_amd.CommitJob(ctx, cols=cols)
    try:
        ptrs = [dev.ptrs[0:3], dev.ptrs[3:5], dev.ptrs[5:6]]
        first = ctx.dev_sumcheck_prove_product_batch(ptrs, ns)  # queued behind the job's build
        roots = job.roots()
        stats, options = ctx.stats(), [ctx.get_option(o) for o in opts]
        second = ctx.dev_sumcheck_prove_product_batch(ptrs, ns)
        third = ctx.sumcheck_prove_product_batch(inst)
        assert ctx.stats() == stats and [ctx.get_option(o) for o in opts] == options
        opened = job.open_all(cexp["points"])
    finally:
        job.end()
        dev.free()
    assert np.array_equal(roots, cexp["roots"])
    for key in ("values", "indices", "leaves", "siblings", "dirs"):
        assert np.array_equal(opened[key], cexp[key]), key
    for got in (first, second, third):
        for g, w in zip(got, ref):
            assert R.same(g, w)
