"""Batched MLE evaluation on the GPU (zigz_dev_mle_eval_batch, zigz_mle_eval_batch): every pair of a batch gives the value of its
own single call, at every size at which the kernel takes another path (one or two elements, less than a chunk, one chunk,
several); the exact u64 sums do not wrap or reduce early; errors come with the first failing pair's index and touch nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
CHUNK = 8192  # MLE_BATCH_CHUNK (kernels.hpp): elements per workgroup
ORACLE_MAX = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


class DevTables:
    """seeded tables uploaded into one device buffer, each 16-byte aligned (offsets in u32 words: multiples of 4)"""

    def __init__(self, ctx, tables, extra_offset=0):
        self.ctx = ctx
        self.off, o = [], extra_offset
        for t in tables:
            self.off.append(o)
            o += (len(t) + 3) // 4 * 4
        packed = np.zeros(max(o, 4), dtype=np.uint64)
        for t, a in zip(tables, self.off):
            packed[a:a + len(t)] = t
        self.base = ctx.dev_alloc(len(packed) * 4)
        ctx.upload(packed, self.base)
        self.ptrs = [self.base + 4 * a for a in self.off]

    def free(self):
        self.ctx.dev_free(self.base)


def _points(seed, ns):
    return [O.splitmix64_field(seed + i, n.bit_length() - 1) if n > 1 else np.zeros(0, np.uint64) for i, n in enumerate(ns)]


def _tables(seed, ns):
    return [O.splitmix64_field(seed + i, n) for i, n in enumerate(ns)]


@pytest.fixture(scope="module")
def small(ctx):
    """every size at which the kernel takes another path, up to 2^17, with the oracle's values (computed once)"""
    ns = [1, 2, 4, 8, 64, 256, 1024, CHUNK // 2, CHUNK, 2 * CHUNK, 1 << 15, 1 << 16, 1 << 17]
    tables, points = _tables(31000, ns), _points(32000, ns)
    exp = [O.mle_eval(P, t, q) for t, q in zip(tables, points)]
    d = DevTables(ctx, tables)
    yield ns, tables, points, exp, d
    d.free()


def test_sizes_where_the_kernel_can_go_wrong(ctx, small):
    ns, tables, points, exp, d = small
    assert ctx.dev_mle_eval_batch(d.ptrs, ns, points) == exp
    assert exp[0] == int(tables[0][0])  # one value: the single entry returns it
    # each pair alone, and in reverse order: a pair's value does not depend on its neighbours or its workgroup numbers
    assert ctx.dev_mle_eval_batch(d.ptrs[::-1], ns[::-1], points[::-1]) == exp[::-1]
    for i in (0, 1, 7, 9):
        assert ctx.dev_mle_eval_batch([d.ptrs[i]], [ns[i]], [points[i]]) == [exp[i]]


def test_host_form_equals_device_form(ctx, small):
    ns, tables, points, exp, d = small
    assert ctx.mle_eval_batch(tables, points) == exp
    assert ctx.mle_eval_batch([], []) == []


def test_mixed_sizes_up_to_2p22(ctx):
    logs = [22, 1, 20, 0, 13, 18, 5, 12, 21, 14, 9, 19, 3, 17, 16, 11]
    ns = [1 << v for v in logs]
    tables, points = _tables(33000, ns), _points(34000, ns)
    d = DevTables(ctx, tables)
    try:
        got = ctx.dev_mle_eval_batch(d.ptrs, ns, points)
        for i, n in enumerate(ns):
            exp = O.mle_eval(P, tables[i], points[i]) if n <= ORACLE_MAX else ctx.dev_mle_eval(d.ptrs[i], n, points[i])
            assert got[i] == exp, (i, n)
    finally:
        d.free()


@pytest.mark.parametrize("n", [2 * CHUNK, 1 << 22])
def test_exact_at_the_bound(ctx, n):
    """every element p - 1: the extension of a constant is that constant, whatever the point -- any wrapped or prematurely
    reduced sum shows, in a shape that spans many workgroups"""
    v = n.bit_length() - 1
    d = DevTables(ctx, [np.full(n, P - 1, dtype=np.uint64)])
    try:
        pts = [np.full(v, P - 1, dtype=np.uint64), np.ones(v, dtype=np.uint64), O.splitmix64_field(35000 + v, v)]
        assert ctx.dev_mle_eval_batch([d.ptrs[0]] * 3, [n] * 3, pts) == [P - 1] * 3
    finally:
        d.free()


def test_repeated_tables(ctx):
    n = 1 << 13
    t = O.splitmix64_field(36000, n)
    pts = [O.splitmix64_field(36100 + i, 13) for i in range(5)]
    pts += [pts[2], pts[2]]
    d = DevTables(ctx, [t], extra_offset=4)  # 16 bytes into the buffer
    try:
        got = ctx.dev_mle_eval_batch([d.ptrs[0]] * 7, [n] * 7, pts)
        assert got == [O.mle_eval(P, t, q) for q in pts]
        assert got[2] == got[5] == got[6]
    finally:
        d.free()


def test_limits(ctx):
    tables = _tables(37000, [2] * 4096)
    points = _points(38000, [2] * 4096)
    d = DevTables(ctx, tables)
    try:
        got = ctx.dev_mle_eval_batch(d.ptrs, [2] * 4096, points)
        for i in range(0, 4096, 97):
            assert got[i] == O.mle_eval(P, tables[i], points[i]), i
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_mle_eval_batch(d.ptrs + d.ptrs[:1], [2] * 4097, points + points[:1])
        assert e.value.code == E.INVALID_ARGUMENT
        assert ctx.dev_mle_eval_batch([], [], []) == []
    finally:
        d.free()


def _raw(ctx, ptrs, ns, points):
    """the raw entry over a prefilled output buffer: (status, bad_index, out)"""
    from zigz_amd._ffi import lib, u64p, vp
    k = len(ns)
    out = np.full(k, 0xABCDEF, dtype=np.uint64)
    q = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64) for x in points] + [np.zeros(1, np.uint64)]))
    bad = C.c_size_t(12345)
    rc = lib.zigz_dev_mle_eval_batch(ctx.h, (vp * k)(*ptrs), (C.c_size_t * k)(*ns), k, q.ctypes.data_as(u64p),
                                     out.ctypes.data_as(u64p), C.byref(bad))
    return rc, bad.value, out


def test_errors_name_the_first_failing_pair_and_touch_nothing(ctx):
    ns = [16, 16, 16, 16]
    tables, points = _tables(39000, ns), _points(39100, ns)
    d = DevTables(ctx, tables)
    try:
        rc, bad, out = _raw(ctx, d.ptrs, ns, points)
        assert rc == 0 and bad == 12345 and out.tolist() == [O.mle_eval(P, t, q) for t, q in zip(tables, points)]
        off4 = list(d.ptrs)
        off4[1] += 4  # 4 bytes off 16-byte alignment
        noncanon = [q.copy() for q in points]
        noncanon[3][2] = P
        for ptrs, nn, pts, code, idx in [(off4, ns, points, E.INVALID_ARGUMENT, 1),
                                         (d.ptrs, [16, 16, 3, 16], [points[0], points[1], points[2][:1], points[3]],
                                          E.LENGTH_NOT_POWER_OF_TWO, 2),
                                         (d.ptrs, [16, 0, 16, 16], [points[0], points[2], points[3]], E.EMPTY_EVALUATIONS, 1),
                                         (d.ptrs, ns, noncanon, E.NOT_CANONICAL, 3)]:
            rc, bad, out = _raw(ctx, ptrs, nn, pts)
            assert (rc, bad) == (code, idx)
            assert np.all(out == 0xABCDEF)
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_mle_eval_batch(off4, ns, points)
        assert e.value.code == E.INVALID_ARGUMENT and e.value.bad_index == 1
    finally:
        d.free()
    bad_t = [t.copy() for t in tables]
    bad_t[2][5] = P + 1
    with pytest.raises(E.ZigzError) as e:
        ctx.mle_eval_batch(bad_t, points)
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 2
    with pytest.raises(E.ZigzError) as e:  # the table before the bad length holds a value >= p: the single calls stop there first
        ctx.mle_eval_batch([tables[0], tables[1], bad_t[2], tables[3][:12]], points)
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 2
    with pytest.raises(E.ZigzError) as e:
        ctx.mle_eval_batch([tables[0], tables[1], tables[2], tables[3][:12]], points)
    assert e.value.code == E.LENGTH_NOT_POWER_OF_TWO and e.value.bad_index == 3


def test_back_to_back_calls_return_their_own_results(ctx, small):
    """a stale completion word, or partial sums left over from the call before, would show in the second call"""
    ns, tables, points, exp, d = small
    other = _points(40000, ns)
    exp2 = [O.mle_eval(P, t, q) for t, q in zip(tables, other)]
    a = ctx.dev_mle_eval_batch(d.ptrs, ns, points)
    b = ctx.dev_mle_eval_batch(d.ptrs[3:], ns[3:], other[3:])
    c = ctx.dev_mle_eval_batch(d.ptrs, ns, other)
    assert a == exp and b == exp2[3:] and c == exp2
