"""Batched Merkle commitments on the GPU (zigz_merkle_commit_batch, zigz_dev_merkle_commit_batch, zigz_merkle_open_batch,
zigz_commit_open_batch): every tree of a batch gives the root, paths, values and indices of its own single call, the error of
the first failing table comes with that table's index, and nothing else on the context is disturbed."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
RAGGED = [1, 2, 3, 5, 255, 256, 257, 1023, 1 << 12, (1 << 15) - 1, (1 << 15) + 1, 1 << 16]


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


def _table(seed, n):
    return O.splitmix64_field(seed, n) if n else np.zeros(0, dtype=np.uint64)


class DevTables:
    """tables uploaded into one device buffer; table i at u32 word offset off[i] (extra_offset words in front of all)"""

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


def _index_sets(ns, seed):
    """four indices per table: 0, n - 1, a random one, and the last real leaf's neighbour inside the padded range"""
    rng = np.random.default_rng(seed)
    rnd = [int(rng.integers(0, n)) for n in ns]
    pad = [n - 2 if n >= 2 and n % 2 == 0 else n - 1 for n in ns]  # n odd: leaf n - 1's sibling is a pad leaf
    return [[0] * len(ns), [n - 1 for n in ns], rnd, pad]


def _single(ctx, t):
    import zigz_amd
    return zigz_amd.SimpleMerkleTree(ctx, t)


def test_commit_batch_matches_oracle(ctx):
    tables = [_table(100 + i, n) for i, n in enumerate(RAGGED)]
    exp = [O.merkle_build(t) for t in tables]
    res, b = ctx.merkle_commit_batch(tables)
    d = DevTables(ctx, tables)
    try:
        dres, db = ctx.dev_merkle_commit_batch(d.ptrs, RAGGED)
    finally:
        d.free()  # the batch owns a copy of the values
    try:
        assert res == exp and dres == exp
        for sel in _index_sets(RAGGED, 7):
            want = [O.merkle_open(t, i) for t, i in zip(tables, sel)]
            for got_all in (b.open(sel), db.open(sel)):
                for g, w, i in zip(got_all, want, sel):
                    assert (g["siblings"], g["directions"], g["value"]) == w and g["index"] == i
    finally:
        b.deinit()
        db.deinit()


def test_large_tables_match_single_calls(ctx):
    ns = [1 << v for v in range(17, 23)] + [(1 << 17) + 3, 1, (1 << 20) - 1]
    tables = [_table(300 + i, n) for i, n in enumerate(ns)]
    res, b = ctx.merkle_commit_batch(tables)
    try:
        sels = _index_sets(ns, 11)
        opened = [b.open(sel) for sel in sels]
        for i, t in enumerate(tables):
            s = _single(ctx, t)
            try:
                assert res[i] == (s.root_hash, s.height)
                for sel, got in zip(sels, opened):
                    w = s.open(sel[i])
                    assert (got[i]["siblings"], got[i]["directions"], got[i]["value"]) == (w["siblings"], w["directions"], w["value"])
            finally:
                s.deinit()
    finally:
        b.deinit()


def test_commit_open_batch_matches_oracle(ctx):
    logs = [0, 1, 2, 5, 8, 9, 10, 11, 12, 13, 14, 16]
    tables = [_table(500 + v, 1 << v) for v in logs]
    rng = np.random.default_rng(3)
    edge = [0, 1, P - 1]
    points = []
    for j, v in enumerate(logs):
        pt = [int(x) for x in rng.integers(0, P, size=v)]
        for c in range(v):  # challenges 0, 1 and p - 1 in every position
            if (c + j) % 4 < 3:
                pt[c] = edge[(c + j) % 4]
        if v and j % 2:
            pt[0] = (1 << v) + 12345 if (1 << v) + 12345 < P else P - 2  # point[0] >= 2^v: the index wraps
        points.append(pt)
    # 2^16 values p - 1 at a random point: the largest exact sum the eight partials of a table can hold before the one reduction
    logs.append(16)
    tables.append(np.full(1 << 16, P - 1, dtype=np.uint64))
    points.append([int(x) for x in rng.integers(0, P, size=16)])
    other = [[int(x) for x in rng.integers(0, P, size=v)] for v in logs]  # a second point set
    ns = [len(t) for t in tables]
    b = db = None
    d = DevTables(ctx, tables, extra_offset=1)  # sources that are only 4-byte aligned: the eval reads the handle's aligned copy
    try:
        try:
            assert d.ptrs[-1] % 16 == 4
            res, b = ctx.merkle_commit_batch(tables)
            dres, db = ctx.dev_merkle_commit_batch(d.ptrs, ns)
        finally:
            d.free()  # the batch owns a copy of the values
        got = ctx.commit_open_batch(b, points)
        again = ctx.commit_open_batch(b, points)  # nothing is carried between calls: no word is zeroed, every one is written
        got_other = ctx.commit_open_batch(b, other)
        back = ctx.commit_open_batch(b, points)
        dgot = ctx.commit_open_batch(db, points)
    finally:
        for h in (b, db):
            if h is not None:
                h.deinit()
    assert again == got
    assert dres == res
    for t, r in zip(tables, res):
        assert r == O.merkle_build(t)
    for pts, runs in ((points, (got, back, dgot)), (other, (got_other,))):
        for i, (t, pt) in enumerate(zip(tables, pts)):
            want = O.commit_open(P, t, pt)
            for run in runs:
                g = run[i]
                assert (g["value"], g["index"], g["siblings"], g["directions"], g["leaf"]) == want


def test_commit_open_batch_large_matches_single_calls(ctx):
    import zigz_amd
    logs = [17, 20, 22, 3]
    tables = [_table(700 + v, 1 << v) for v in logs]
    rng = np.random.default_rng(5)
    points = [[int(x) for x in rng.integers(0, P, size=v)] for v in logs]
    _, b = ctx.merkle_commit_batch(tables)
    try:
        got = ctx.commit_open_batch(b, points)
    finally:
        b.deinit()
    for t, pt, g in zip(tables, points, got):
        s = _single(ctx, t)
        try:
            w = zigz_amd.CommitmentScheme.open(ctx, t, s, pt)
        finally:
            s.deinit()
        assert g == w


def test_degenerate_batches(ctx):
    one = _table(1, 1000)
    res, b = ctx.merkle_commit_batch([one])
    b.deinit()
    assert res == [O.merkle_build(one)]
    assert ctx.merkle_commit_batch([]) == ([], None)
    # 4096 tables of mixed small sizes, roots only
    ns = [1 + (i * 37) % 700 for i in range(4096)]
    tables = [_table(i, n) for i, n in enumerate(ns)]
    res, none = ctx.merkle_commit_batch(tables, keep=False)
    assert none is None
    for i in (0, 1, 2, 1000, 4095):
        assert res[i] == O.merkle_build(tables[i])
    with pytest.raises(E.ZigzError) as e:
        ctx.merkle_commit_batch(tables + [one])
    assert e.value.code == E.INVALID_ARGUMENT
    # the same device table three times, and a table at a 4-byte offset (only 4-byte aligned)
    t = _table(9, 777)
    d = DevTables(ctx, [t, _table(10, 5)], extra_offset=1)
    try:
        assert d.ptrs[0] % 16 == 4
        dres, db = ctx.dev_merkle_commit_batch([d.ptrs[0], d.ptrs[1], d.ptrs[0], d.ptrs[0]], [777, 5, 777, 300])
        try:
            opened = db.open([776, 4, 0, 299])
        finally:
            db.deinit()
    finally:
        d.free()
    assert dres[0] == dres[2] == O.merkle_build(t) and dres[3] == O.merkle_build(t[:300])
    assert dres[1] == O.merkle_build(_table(10, 5))
    assert (opened[0]["siblings"], opened[0]["directions"], opened[0]["value"]) == O.merkle_open(t, 776)
    assert (opened[3]["siblings"], opened[3]["directions"], opened[3]["value"]) == O.merkle_open(t[:300], 299)


def test_errors_name_the_first_failing_table(ctx):
    from zigz_amd._ffi import lib, u64p, u8p
    tables = [_table(40 + i, 64) for i in range(4)]
    # n = 0 in table 2: nothing runs, the outputs stay as they were
    ns = (C.c_size_t * 4)(64, 64, 0, 64)
    ptrs = (u64p * 4)(*[t.ctypes.data_as(u64p) for t in tables])
    roots = np.full(4 * 32, 0xAB, dtype=np.uint8)
    heights = (C.c_size_t * 4)(7, 7, 7, 7)
    h, bad = C.c_void_p(), C.c_size_t(99)
    rc = lib.zigz_merkle_commit_batch(ctx.h, ptrs, ns, 4, roots.ctypes.data_as(u8p), heights, C.byref(h), C.byref(bad))
    assert (rc, bad.value) == (E.EMPTY_VALUES, 2)
    assert (roots == 0xAB).all() and list(heights) == [7] * 4 and not h.value
    # a value >= p: the first table holding one, even before a table that fails its length check
    badt = [t.copy() for t in tables]
    badt[1][63] = P
    for call, idx in [([tables[0], badt[1], tables[2]], 1), ([tables[0], badt[1], np.zeros(0, np.uint64)], 1),
                      ([tables[0], tables[1], np.zeros(0, np.uint64), badt[1]], 2)]:
        with pytest.raises(E.ZigzError) as e:
            ctx.merkle_commit_batch(call)
        assert e.value.bad_index == idx
        assert e.value.code == (E.NOT_CANONICAL if idx == 1 else E.EMPTY_VALUES)
    # an index out of range; a table that is not a power of two in commit_open_batch; a coordinate >= p
    mixed = [tables[0], tables[1][:48], tables[2]]
    _, b = ctx.merkle_commit_batch(mixed)
    try:
        with pytest.raises(E.ZigzError) as e:
            b.open([0, 48, 0])
        assert (e.value.code, e.value.bad_index) == (E.INDEX_OUT_OF_BOUNDS, 1)
        with pytest.raises(E.ZigzError) as e:
            ctx.commit_open_batch(b, [[1] * 6, [2] * 6, [3] * 6])
        assert (e.value.code, e.value.bad_index) == (E.LENGTH_NOT_POWER_OF_TWO, 1)
        got = b.open([63, 47, 5])  # the context and the batch still work
        for g, t, i in zip(got, mixed, [63, 47, 5]):
            assert (g["siblings"], g["directions"], g["value"]) == O.merkle_open(t, i)
    finally:
        b.deinit()
    _, b = ctx.merkle_commit_batch(tables[:3])
    try:
        with pytest.raises(E.ZigzError) as e:
            ctx.commit_open_batch(b, [[1] * 6, [2] * 6, [3, 4, 5, P, 0, 0]])
        assert (e.value.code, e.value.bad_index) == (E.NOT_CANONICAL, 2)
    finally:
        b.deinit()


def test_batch_while_a_commit_job_is_active(ctx):
    import zigz_amd
    nv = 11
    cols = np.stack([O.splitmix64_field(6000 + c, 1 << nv) for c in range(43)])
    cexp = O.generate_commitments(P, O.Transcript(), cols, fast=True)
    ns = [1, 256, 1 << 10, 4096, 1 << 14]
    tables = [_table(800 + i, n) for i, n in enumerate(ns)]
    exp = [O.merkle_build(t) for t in tables]
    sel = [0, 255, 1000, 4095, 12345]
    wopen = [O.merkle_open(t, i) for t, i in zip(tables, sel)]
    pts = [[int(x) for x in O.splitmix64_field(900 + i, n.bit_length() - 1)] for i, n in enumerate(ns)]
    wco = [O.commit_open(P, t, p) for t, p in zip(tables, pts)]
    job = zigz_amd.CommitJob(ctx, cols=cols)
    try:
        res1, b1 = ctx.merkle_commit_batch(tables)  # queued behind the job's build
        roots = job.roots()
        before = ctx.stats()
        res2, b2 = ctx.merkle_commit_batch(tables)
        o1, o2 = b1.open(sel), b2.open(sel)
        co = ctx.commit_open_batch(b2, pts)
        after = ctx.stats()
        opened = job.open_all(cexp["points"])
        b1.deinit()
        b2.deinit()
    finally:
        job.end()
    assert before == after
    assert np.array_equal(roots, cexp["roots"])
    for key in ("values", "indices", "leaves", "siblings", "dirs"):
        assert np.array_equal(opened[key], cexp[key]), key
    assert res1 == exp and res2 == exp
    for got in (o1, o2):
        for g, w in zip(got, wopen):
            assert (g["siblings"], g["directions"], g["value"]) == w
    for g, w in zip(co, wco):
        assert (g["value"], g["index"], g["siblings"], g["directions"], g["leaf"]) == w


def test_two_contexts_run_batches_concurrently(ctx):
    import zigz_amd
    sets = [[_table(1000 * c + i, n) for i, n in enumerate([3, 700, 1 << 12, 9000, 1 << 15])] for c in range(2)]
    exp = [[O.merkle_build(t) for t in s] for s in sets]
    out, errs = [None, None], []

    def run(c):
        try:
            cx = zigz_amd.Context(0)
            got = []
            for _ in range(5):
                res, b = cx.merkle_commit_batch(sets[c])
                got.append((res, b.open([1, 2, 3, 4, 5])))
                b.deinit()
            out[c] = got
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    th = [threading.Thread(target=run, args=(c,)) for c in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for c in range(2):
        w = [O.merkle_open(t, i) for t, i in zip(sets[c], [1, 2, 3, 4, 5])]
        for res, opened in out[c]:
            assert res == exp[c]
            for g, ww in zip(opened, w):
                assert (g["siblings"], g["directions"], g["value"]) == ww
