"""Many openings per committed tree on the GPU (zigz_merkle_open_many, zigz_dev_merkle_open_many, zigz_commit_open_many):
every sibling, direction, leaf, root and height is the oracle's (merkle_open / merkle_build) for that tree and index, in the
packed layout the batched verify entries read; the host form in several chunks, the device form straight into the verifier;
errors name the first offender and write nothing; nothing else on the context is disturbed; and the commit-job form reads
list-built, content-addressed and virtual-leaf trees as well as dense ones, single and batched."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
SMALL_NS = [1, 2, 3, 5, 8, 257, 4097]
SMALL_HS = [0, 1, 2, 3, 3, 9, 13]
VERIFY_MAX = 1 << 22
# the hints a prover gives for the 43 witness columns (small-domain, run-aware, content-addressed group)
HINTS = {"small_domain_mask": (1 << 1) | (0x3f << 33) | (1 << 42), "run_aware_mask": (0x7fffffff << 2) | (3 << 40),
         "cons_group_mask": 1 | (1 << 1) | (0x7f << 33) | (1 << 42)}


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    c = zigz_amd.Context(0)
    yield c


@pytest.fixture(scope="module")
def E():
    from zigz_amd import errors
    return errors


def _table(seed, n):
    return O.splitmix64_field(seed, n)


class Memo:
    """oracle openings, each computed once (equal columns share theirs)"""

    def __init__(self):
        self.m = {}

    def open(self, values, index):
        key = (values.tobytes(), int(index))
        if key not in self.m:
            self.m[key] = O.merkle_open(values, int(index))
        return self.m[key]


def _expect(memo, tables, trees, indices):
    """the packed arrays the oracle gives for these openings"""
    sib, dirs, leaves, roots, hs = [], [], [], [], []
    built = {}
    for t, i in zip(trees, indices):
        s, d, leaf = memo.open(tables[t], i)
        if t not in built:
            built[t] = O.merkle_build(tables[t])
        sib.append(s)
        dirs.append(d)
        leaves.append(leaf)
        roots.append(built[t][0])
        hs.append(built[t][1])
    return dict(siblings=np.frombuffer(b"".join(sib), dtype=np.uint8), dirs=np.frombuffer(b"".join(dirs), dtype=np.uint8),
                leaves=np.array(leaves, dtype=np.uint64), roots=np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(-1, 32),
                heights=np.array(hs, dtype=np.int64))


def _same(got, want, what=""):
    for key in ("heights", "leaves", "dirs", "roots", "siblings"):
        assert np.array_equal(got[key], want[key]), (what, key)


class DevOut:
    """device arrays for the device form, prefilled with 0xEE"""

    def __init__(self, k, tot):
        import torch
        self.k, self.tot = k, tot
        self.sib = torch.full((32 * tot + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        self.dirs = torch.full((tot + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        self.leaf = torch.full((k + 8,), -1, dtype=torch.int64, device="cuda")
        self.roots = torch.full((32 * k + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the library runs on its own stream)

    def ptrs(self):
        return self.sib.data_ptr(), self.dirs.data_ptr(), self.leaf.data_ptr(), self.roots.data_ptr()

    def host(self, heights):
        k, tot = self.k, self.tot
        return dict(siblings=self.sib.cpu().numpy()[: 32 * tot], dirs=self.dirs.cpu().numpy()[:tot],
                    leaves=self.leaf.cpu().numpy().view(np.uint64)[:k], roots=self.roots.cpu().numpy()[: 32 * k].reshape(k, 32),
                    heights=heights)


def _dev_open(ctx, b, trees, indices):
    tot = int(sum(b.heights[t] for t in trees))
    out = DevOut(len(trees), tot)
    hs = b.dev_open_many(trees, indices, *out.ptrs())
    ctx.synchronize()
    return out.host(hs), out


@pytest.fixture(scope="module")
def small(ctx):
    tables = [_table(100 + i, n) for i, n in enumerate(SMALL_NS)]
    res, b = ctx.merkle_commit_batch(tables)
    assert [h for _, h in res] == SMALL_HS
    yield tables, res, b
    b.deinit()


def test_every_small_shape(ctx, small):
    tables, res, b = small
    rng = np.random.default_rng(1)
    pairs = [(t, i) for t in range(6) for i in range(SMALL_NS[t])]
    last = [0, 4096] + [int(x) for x in rng.integers(0, 4097, size=62)]
    pairs += [(6, i) for i in last]
    pairs += [pairs[int(x)] for x in rng.integers(0, len(pairs), size=9)]  # a few pairs repeated
    order = rng.permutation(len(pairs))  # heights mix inside a wave
    trees = [pairs[j][0] for j in order]
    indices = [pairs[j][1] for j in order]
    want = _expect(Memo(), tables, trees, indices)
    assert [r for r, _ in res] == [O.merkle_build(t)[0] for t in tables]
    _same(b.open_many(trees, indices), want, "host form")
    got, _ = _dev_open(ctx, b, trees, indices)
    _same(got, want, "device form")
    # every opening is zigz_merkle_open_batch's for that tree and index
    one = b.open([0, 1, 2, 4, 7, 256, 4096])
    many = b.open_many(list(range(7)), [0, 1, 2, 4, 7, 256, 4096])
    assert many["siblings"].tobytes() == b"".join(o["siblings"] for o in one)
    assert many["dirs"].tobytes() == b"".join(o["directions"] for o in one)
    assert many["leaves"].tolist() == [o["value"] for o in one]
    # only openings without siblings: siblings and dirs may be NULL
    from zigz_amd._ffi import lib, u32p, u64p, u8p
    t0 = np.zeros(3, dtype=np.uint32)
    i0 = np.zeros(3, dtype=np.uint64)
    leaf = np.zeros(3, dtype=np.uint64)
    roots = np.zeros(96, dtype=np.uint8)
    assert lib.zigz_merkle_open_many(ctx.h, b.h, 3, t0.ctypes.data_as(u32p), i0.ctypes.data_as(u64p), None, None,
                                     leaf.ctypes.data_as(u64p), roots.ctypes.data_as(u8p), None, None) == 0
    assert leaf.tolist() == [int(tables[0][0])] * 3 and roots.tobytes() == res[0][0] * 3


def test_many_openings_in_several_chunks(ctx):
    n, k = 1 << 13, (1 << 17) + 3  # 54.5 MB of siblings: past one 32 MiB chunk
    values = _table(200, n)
    res, b = ctx.merkle_commit_batch([values])
    try:
        rng = np.random.default_rng(2)
        indices = rng.integers(0, n, size=k).astype(np.uint64)
        got = b.open_many(np.zeros(k, dtype=np.uint32), indices)
    finally:
        b.deinit()
    assert got["heights"].tolist() == [13] * k
    assert np.array_equal(got["dirs"].reshape(k, 13), ((indices[:, None] >> np.arange(13, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8))
    assert np.array_equal(got["leaves"], values[indices])
    assert np.array_equal(got["roots"], np.tile(np.frombuffer(res[0][0], dtype=np.uint8), (k, 1)))
    sib = got["siblings"].reshape(k, 13 * 32)
    for j in [0, k - 1] + [int(x) for x in rng.integers(0, k, size=62)]:
        s, d, leaf = O.merkle_open(values, int(indices[j]))
        assert sib[j].tobytes() == s and got["dirs"][13 * j: 13 * j + 13].tobytes() == d and int(got["leaves"][j]) == leaf, j
    verd = ctx.merkle_verify_batch(got["roots"], got["heights"], got["leaves"], got["siblings"], got["dirs"])
    assert int((verd == 0).sum()) == 0 and len(verd) == k


def test_open_to_verify_on_the_device(ctx, small, E):
    import torch
    tables, res, b = small
    rng = np.random.default_rng(3)
    trees = [int(x) for x in rng.integers(0, 7, size=500)]
    indices = [int(rng.integers(0, SMALL_NS[t])) for t in trees]
    got, out = _dev_open(ctx, b, trees, indices)
    sib, dirs, leaf, roots = out.ptrs()
    verd = ctx.dev_merkle_verify_batch(roots, got["heights"], leaf, sib, dirs)
    assert verd.tolist() == [1] * 500
    j = next(x for x in range(100, 500) if SMALL_HS[trees[x]] >= 2)
    off = int(sum(SMALL_HS[t] for t in trees[:j]))
    out.sib[32 * (off + 1) + 7] ^= 1  # one byte of opening j's second sibling
    torch.cuda.synchronize()
    verd = ctx.dev_merkle_verify_batch(roots, got["heights"], leaf, sib, dirs)
    assert verd.tolist() == [0 if x == j else 1 for x in range(500)]
    with pytest.raises(E.ZigzError) as e:
        b.dev_open_many(trees, indices, sib + 8, dirs, leaf, roots)
    assert e.value.code == E.INVALID_ARGUMENT
    with pytest.raises(E.ZigzError) as e:
        b.dev_open_many(trees, indices, sib, dirs, leaf + 4, roots)
    assert e.value.code == E.INVALID_ARGUMENT


def test_errors_write_nothing(ctx, small, E):
    import zigz_amd
    from zigz_amd._ffi import lib, u32p, u64p, u8p
    tables, res, b = small

    def raw(k, trees, indices, batch=b, c=ctx):
        t = np.asarray(trees, dtype=np.uint32)
        ix = np.asarray(indices, dtype=np.uint64)
        outs = [np.full(32 * 64, 0xCD, dtype=np.uint8), np.full(64, 0xCD, dtype=np.uint8), np.full(8, 0xCDCDCDCD, dtype=np.uint64),
                np.full(32 * 8, 0xCD, dtype=np.uint8)]
        hs = (C.c_size_t * 8)(*([777] * 8))
        bad = C.c_size_t(99)
        rc = lib.zigz_merkle_open_many(c.h, batch.h, k, t.ctypes.data_as(u32p), ix.ctypes.data_as(u64p), outs[0].ctypes.data_as(u8p),
                                       outs[1].ctypes.data_as(u8p), outs[2].ctypes.data_as(u64p), outs[3].ctypes.data_as(u8p), hs,
                                       C.byref(bad))
        clean = all((o == o.dtype.type(0xCDCDCDCD if o.dtype == np.uint64 else 0xCD)).all() for o in outs) and list(hs) == [777] * 8
        return rc, bad.value, clean

    # a tree id equal to the table count -- at 2 and at 3 -- and an index equal to n of the 4097-value table (4096 is valid)
    assert raw(4, [0, 6, 7, 7], [0, 4096, 0, 0]) == (E.INVALID_ARGUMENT, 2, True)
    assert raw(4, [6, 6, 6, 6], [4096, 4097, 0, 4097]) == (E.INDEX_OUT_OF_BOUNDS, 1, True)
    assert raw(3, [2, 2, 2], [2, 3, 3]) == (E.INDEX_OUT_OF_BOUNDS, 1, True)  # n = 3 of a tree padded to 4
    assert raw(0, [0], [0]) == (0, 99, True)
    assert raw(VERIFY_MAX + 1, [0], [0]) == (E.INVALID_ARGUMENT, 99, True)  # (refused before trees[1..] would be read)
    rc, bad, clean = raw(4, [0, 6, 5, 1], [0, 4096, 256, 1])
    assert (rc, bad, clean) == (0, 99, False)
    other = zigz_amd.Context(0)
    try:
        assert raw(1, [0], [0], c=other) == (E.INVALID_ARGUMENT, 99, True)  # a batch of another context
    finally:
        other.close()
    with pytest.raises(E.ZigzError) as e:
        b.open_many([0, 7, 9], [0, 0, 0])
    assert (e.value.code, e.value.bad_index) == (E.INVALID_ARGUMENT, 1)
    with pytest.raises(E.ZigzError) as e:
        _dev_open(ctx, b, [5, 5], [256, 257])
    assert (e.value.code, e.value.bad_index) == (E.INDEX_OUT_OF_BOUNDS, 1)
    # NULL arrays
    t = np.zeros(2, dtype=np.uint32)
    ix = np.zeros(2, dtype=np.uint64)
    o8 = np.zeros(256, dtype=np.uint8)
    o64 = np.zeros(8, dtype=np.uint64)
    good = [t.ctypes.data_as(u32p), ix.ctypes.data_as(u64p), o8.ctypes.data_as(u8p), o8.ctypes.data_as(u8p), o64.ctypes.data_as(u64p)]
    t[:] = 3
    for i in range(5):
        a = list(good)
        a[i] = None
        assert lib.zigz_merkle_open_many(ctx.h, b.h, 2, *a, None, None, None) == E.INVALID_ARGUMENT, i
    assert lib.zigz_merkle_open_many(None, b.h, 2, *good, None, None, None) == E.INVALID_ARGUMENT
    assert lib.zigz_merkle_open_many(ctx.h, None, 2, *good, None, None, None) == E.INVALID_ARGUMENT
    assert lib.zigz_merkle_open_many(ctx.h, b.h, 2, *good, None, None, None) == 0  # roots, heights and bad_index may be NULL


@pytest.fixture(scope="module")
def witness():
    """a looping program's 43 witness columns of 2^15 rows, the oracle's commitments, and a memo of oracle openings"""
    import programs
    from zigz_amd import host
    N = 1 << 15
    tr = host.Trace(programs.add_xor_loop((N - 3) // 4), 0x1000, None, 2 * N)
    assert tr.num_vars == 15
    cols = tr.witness()
    return cols, O.generate_commitments(P, O.Transcript(), cols, fast=True), Memo()


class Hints:
    def __init__(self, ctx, on=True):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        self.saved = {k: self.ctx.get_option(k) for k in HINTS}
        for k, v in HINTS.items():
            self.ctx.set_option(k, v if self.on else 0)
        self.ctx.set_option("cons_always", 1 if self.on else 0)

    def __exit__(self, *a):
        self.ctx.set_option("cons_always", 0)
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)


def test_the_context_is_left_alone(ctx, small, witness):
    import zigz_amd
    tables, _, b = small
    cols, cexp, _ = witness
    trees, indices = [6, 0, 5, 6, 3], [4096, 0, 17, 1, 4]
    want = _expect(Memo(), tables, trees, indices)
    with Hints(ctx):
        job = zigz_amd.CommitJob(ctx, cols=cols)
        try:
            base_roots = job.roots()
            base = job.open_all(cexp["points"])
        finally:
            job.end()
        job = zigz_amd.CommitJob(ctx, cols=cols)
        try:
            for where in ("before roots", "after roots"):
                opts, stats = {k: ctx.get_option(k) for k in HINTS}, ctx.stats()
                _same(b.open_many(trees, indices), want, where)
                got, _ = _dev_open(ctx, b, trees, indices)
                _same(got, want, where)
                assert {k: ctx.get_option(k) for k in HINTS} == opts and ctx.stats() == stats, where
                if where == "before roots":
                    roots = job.roots()
            opened = job.open_all(cexp["points"])
        finally:
            job.end()
    assert np.array_equal(roots, base_roots) and np.array_equal(roots, cexp["roots"])
    for key in ("values", "indices", "leaves", "siblings", "dirs"):
        assert np.array_equal(opened[key], base[key]) and np.array_equal(opened[key], cexp[key]), key
    # other open batches are left alone too
    assert b.open([0, 1, 2, 4, 7, 256, 4096])[6]["siblings"] == O.merkle_open(tables[6], 4096)[0]


def _job_expect(memo, cols, pairs):
    sib, dirs, leaves = [], [], []
    for c, i in pairs:
        s, d, leaf = memo.open(cols[c], i)
        sib.append(np.frombuffer(s, dtype=np.uint8).reshape(-1, 32))
        dirs.append(np.frombuffer(d, dtype=np.uint8))
        leaves.append(leaf)
    return dict(siblings=np.stack(sib), dirs=np.stack(dirs), leaves=np.array(leaves, dtype=np.uint64))


def test_commit_job_form(ctx, witness, E):
    import zigz_amd
    cols, cexp, memo = witness
    N = 1 << 15
    rng = np.random.default_rng(6)
    seeded = [int(x) for x in rng.integers(0, N, size=4)]
    pairs = [(c, i) for c in range(43) for i in seeded + [0, N - 1]]
    pairs = [pairs[j] for j in rng.permutation(len(pairs))]
    want = _job_expect(memo, cols, pairs)
    got = {}
    for hinted in (True, False):
        with Hints(ctx, hinted):
            job = zigz_amd.CommitJob(ctx, cols=cols)
            try:
                with pytest.raises(E.ZigzError) as e:
                    job.open_many([0], [0])  # before roots
                assert e.value.code == E.BAD_STATE
                assert np.array_equal(job.roots(), cexp["roots"])
                st = ctx.stats()
                if hinted:  # list-built trees, the content-addressed group and virtual leaves are in play
                    assert st["run_aware_columns"] == 33 and st["cons_columns"] == 10, st
                else:
                    assert st["run_aware_columns"] == 0 and st["cons_columns"] == 0 and st["small_domain_columns"] == 0, st
                got[hinted] = job.open_many([c for c, _ in pairs], [i for _, i in pairs])
                opened = job.open_all(cexp["points"])
                again = job.open_many([c for c, _ in pairs[:50]], [i for _, i in pairs[:50]])  # after open_all as well
                with pytest.raises(E.ZigzError) as e:
                    job.open_many([0, 43, 43], [0, 0, 0])
                assert (e.value.code, e.value.bad_index) == (E.INVALID_ARGUMENT, 1)
                with pytest.raises(E.ZigzError) as e:
                    job.open_many([0, 1, 2], [N - 1, 0, N])
                assert (e.value.code, e.value.bad_index) == (E.INDEX_OUT_OF_BOUNDS, 2)
                assert len(job.open_many([], [])["leaves"]) == 0
            finally:
                job.end()
            with pytest.raises(E.ZigzError) as e:
                job.open_many([0], [0])  # after end
            assert e.value.code == E.BAD_STATE
        for key in ("values", "indices", "leaves", "siblings", "dirs"):
            assert np.array_equal(opened[key], cexp[key]), (hinted, key)
        for key in ("leaves", "dirs", "siblings"):
            assert np.array_equal(got[hinted][key], want[key]), (hinted, key)
            assert np.array_equal(again[key], want[key][:50]), (hinted, key, "after open_all")
    for key in ("leaves", "dirs", "siblings"):
        assert np.array_equal(got[True][key], got[False][key]), key


def _trace_cols(ctx, prog, nv):
    """a program's witness columns, host and device"""
    from zigz_amd import host
    tr = host.Trace(prog, 0x1000, None, 1 << 20)
    assert tr.num_vars == nv, (tr.num_vars, nv)
    N = 1 << nv
    d = ctx.dev_alloc(43 * N * 4)
    tr.witness_to_device(ctx, d, N)
    return tr.witness(), d


@pytest.mark.parametrize("nv,hinted", [(10, False), (15, True)])
def test_commit_job_form_of_a_batched_job(ctx, nv, hinted):
    """two proofs in one job: flat and dense at 2^10, in arenas with structure-aware trees at 2^15 (every pointer of the
    second proof's trees moves by the arena stride); columns of both proofs interleaved in one call"""
    import programs
    import zigz_amd
    N = 1 << nv
    progs = [programs.add_xor_loop((N - 3) // 4), programs.add_xor_loop((N - 3) // 4 - 5)]
    bufs = []
    memo = Memo()
    rng = np.random.default_rng(nv)
    try:
        for p_ in progs:
            bufs.append(_trace_cols(ctx, p_, nv))
        both = np.concatenate([h for h, _ in bufs])  # the job's column numbering: proof by proof
        if nv == 10:
            pairs = [(c, i) for c in range(86) for i in (0, N - 1, int(rng.integers(0, N)))]
        else:  # a group column, a small-domain one, run-aware registers, a dense one -- of each proof
            pairs = [(c + 43 * z, i) for z in (0, 1) for c in (0, 1, 5, 34, 41, 42) for i in (0, N - 1, int(rng.integers(0, N)))]
        pairs = [pairs[j] for j in rng.permutation(len(pairs))]
        want = _job_expect(memo, both, pairs)
        with Hints(ctx, hinted):
            job = zigz_amd.CommitJob(ctx, d_cols_list=[d for _, d in bufs], ncols=43, nv=nv, col_stride=N)
            try:
                roots = job.roots()
                got = job.open_many([c for c, _ in pairs], [i for _, i in pairs])
            finally:
                job.end()
        for c in {c for c, _ in pairs}:
            assert roots[c].tobytes() == O.merkle_build(both[c])[0], c
        for key in ("leaves", "dirs", "siblings"):
            assert np.array_equal(got[key], want[key]), key
    finally:
        for _, d in bufs:
            ctx.dev_free(d)
