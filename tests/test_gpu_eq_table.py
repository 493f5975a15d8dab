"""Batched eq tables on the GPU (zigz_dev_eq_table_batch, zigz_eq_table_batch): every word equals the table built from the
definition in numpy (zerocheck_ref.eq_table), at every length at which k_eq_batch_expand takes another path, for random and
edge taus; nothing behind a table is written; the batched eval -- an independent kernel -- agrees; argument errors write
nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import zerocheck_ref as Z

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
# 1, 2: no 16-byte store; 4: one store, one lane; 2^9: partial chunk, A and B with missing variables; 2^12: partial loop; 2^13: one
# chunk exactly; 2^14: H has one factor; 2^20: 128 workgroups
LENGTHS = [1, 2, 4, 1 << 9, 1 << 12, 1 << 13, 1 << 14, 1 << 20]
GUARD = 16  # words behind every table (64 bytes), pre-filled
FILL = 0x5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


def taus(v, seed):
    rnd = [int(x) for x in O.splitmix64_field(seed, v)]
    return {"random": rnd, "zero": [0] * v, "one": [1] * v, "pm1": [P - 1] * v, "bits": [(j * 5 + 1) % 3 % 2 for j in range(v)]}


_REF = {}


def ref(tau):
    """the numpy table of a tau, computed once"""
    key = tuple(tau)
    if key not in _REF:
        _REF[key] = Z.eq_table(tau)
    return _REF[key]


def build(ctx, ns, points, calls=1):
    """runs dev_eq_table_batch into one pre-filled device buffer (every table 16-byte aligned with GUARD words behind it) and
    returns the downloaded tables and guards"""
    offs, o = [], 0
    for n in ns:
        offs.append(o)
        o += (n + GUARD + 3) // 4 * 4
    base = ctx.dev_alloc(o * 4)
    try:
        ctx.upload(np.full(o, FILL, dtype=np.uint64), base)
        for _ in range(calls):
            ctx.dev_eq_table_batch([base + 4 * a for a in offs], ns, points)
        words = ctx.download(base, o)
    finally:
        ctx.dev_free(base)
    return [words[a: a + n] for a, n in zip(offs, ns)], [words[a + n: a + n + GUARD] for a, n in zip(offs, ns)]


@pytest.mark.parametrize("n", LENGTHS)
def test_every_word_equals_the_definition(ctx, n):
    v = n.bit_length() - 1
    ts = list(taus(v, 9100 + v).values())
    tabs, guards = build(ctx, [n] * len(ts), ts)
    for tau, t, g in zip(ts, tabs, guards):
        assert np.array_equal(t, ref(tau)), tau[:4]
        assert np.all(g == FILL)


def test_mixed_sizes_ascending_and_descending_twice(ctx):
    ns = LENGTHS + LENGTHS[::-1]
    ts = [taus(n.bit_length() - 1, 9100 + n.bit_length() - 1)["random"] for n in ns]
    tabs, guards = build(ctx, ns, ts, calls=2)
    for tau, t, g in zip(ts, tabs, guards):
        assert np.array_equal(t, ref(tau)), len(t)
        assert np.all(g == FILL)


def test_4096_tables(ctx):
    k, v = 4096, 10
    pts = O.splitmix64_field(9200, k * v).reshape(k, v)
    tabs, guards = build(ctx, [1 << v] * k, [list(p) for p in pts])
    for i in list(range(0, k, 97)) + [k - 1]:
        assert np.array_equal(tabs[i], Z.eq_table(pts[i])), i
    # every table sums to 1, whichever its tau
    assert all(int(np.sum(t, dtype=np.uint64)) % P == 1 for t in tabs)
    assert all(np.all(g == FILL) for g in guards)


def test_host_form_equals_the_device_form(ctx):
    ns = [1, 1 << 9, 1 << 14]
    ts = [taus(n.bit_length() - 1, 9300 + i)["random"] for i, n in enumerate(ns)]
    dev, _ = build(ctx, ns, ts)
    host = ctx.eq_table_batch(ns, ts)
    for a, b, tau in zip(dev, host, ts):
        assert b.dtype == np.uint64 and np.array_equal(a, b) and np.array_equal(b, ref(tau))
    assert ctx.eq_table_batch([], []) == []


@pytest.mark.parametrize("n", [1 << 13, 1 << 20])
def test_the_batched_eval_agrees(ctx, n):
    """dev_mle_eval_batch(T, tau) -- k_mle_batch_eval, which forms the same weights and adds them up -- equals sum E_tau T over
    the DOWNLOADED table"""
    v = n.bit_length() - 1
    tau = taus(v, 9400 + v)["random"]
    t = O.splitmix64_field(9500 + v, n)
    (e,), _ = build(ctx, [n], [tau])
    d = ctx.dev_alloc(n * 4)
    try:
        ctx.upload(t, d)
        assert ctx.dev_mle_eval_batch([d], [n], [tau]) == [Z.dot(e, t)]
    finally:
        ctx.dev_free(d)


def test_argument_errors_write_nothing(ctx):
    from zigz_amd._ffi import lib, u64p, vp
    ns = [4, 8, 2, 16]
    k, tot = len(ns), 128  # bytes: the four tables at offs, each 16-byte aligned
    pts = np.ascontiguousarray(O.splitmix64_field(9600, 10))
    base = ctx.dev_alloc(tot)
    host = [np.full(n, FILL, dtype=np.uint64) for n in ns]
    offs = [0, 16, 48, 64]

    def raw(dev, nn, points=pts, shift=None, null=None, kk=k):
        ctx.upload(np.full(tot // 4, FILL, dtype=np.uint64), base)
        for h in host:
            h[:] = FILL
        bad = C.c_size_t(12345)
        sz = (C.c_size_t * k)(*nn)
        pp = None if points is None else points.ctypes.data_as(u64p)
        if dev:
            ptrs = [base + o + (4 if shift == i else 0) for i, o in enumerate(offs)]
            arr = (vp * k)(*[None if null == i else p for i, p in enumerate(ptrs)])
            rc = lib.zigz_dev_eq_table_batch(ctx.h, kk, sz, pp, arr, C.byref(bad))
            untouched = bool(np.all(ctx.download(base, tot // 4) == FILL))
        else:
            arr = (u64p * k)(*[None if null == i else h.ctypes.data_as(u64p) for i, h in enumerate(host)])
            rc = lib.zigz_eq_table_batch(ctx.h, kk, sz, pp, arr, C.byref(bad))
            untouched = all(bool(np.all(h == FILL)) for h in host)
        return rc, bad.value, untouched

    try:
        for dev in (True, False):
            assert raw(dev, ns) == (0, 12345, False)
            assert raw(dev, ns, kk=0) == (0, 12345, True)
            assert raw(dev, ns, kk=4097) == (E.INVALID_ARGUMENT, 12345, True)
            assert raw(dev, ns, points=None) == (E.INVALID_ARGUMENT, 12345, True)
            assert raw(dev, ns, null=2) == (E.INVALID_ARGUMENT, 2, True)
            assert raw(dev, [4, 8, 2, 1 << 33]) == (E.INVALID_ARGUMENT, 3, True)
            assert raw(dev, [4, 6, 2, 16]) == (E.LENGTH_NOT_POWER_OF_TWO, 1, True)
            assert raw(dev, [4, 0, 2, 16]) == (E.EMPTY_EVALUATIONS, 1, True)
            bad_pts = pts.copy()
            bad_pts[2 + 3] = P  # table 2's coordinate, behind a later table's bad length
            assert raw(dev, [4, 8, 2, 12], points=bad_pts) == (E.NOT_CANONICAL, 2, True)
            # 2^24 chunks or more in one call (32 tables of 2^32): rejected before anything is built or written
            big, zeros, bad = (C.c_size_t * 32)(*[1 << 32] * 32), np.zeros(32 * 32, dtype=np.uint64), C.c_size_t(12345)
            if dev:
                rc = lib.zigz_dev_eq_table_batch(ctx.h, 32, big, zeros.ctypes.data_as(u64p), (vp * 32)(*[base] * 32), C.byref(bad))
            else:
                rc = lib.zigz_eq_table_batch(ctx.h, 32, big, zeros.ctypes.data_as(u64p), (u64p * 32)(*[host[0].ctypes.data_as(u64p)] * 32),
                                             C.byref(bad))
            assert (rc, bad.value) == (E.INVALID_ARGUMENT, 12345)
        assert raw(True, ns, shift=1) == (E.INVALID_ARGUMENT, 1, True)
        assert lib.zigz_dev_eq_table_batch(None, k, None, None, None, None) == E.INVALID_ARGUMENT
    finally:
        ctx.dev_free(base)
