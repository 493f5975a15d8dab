"""Batched Merkle verification on the GPU (zigz_merkle_verify_batch, zigz_dev_merkle_verify_batch, Context.commit_verify_batch,
CommitmentScheme::batchVerify(ctx, ...)): every verdict is SimpleMerkleTree.verify's on the same bytes -- honest openings from
the oracle and from the batched openings are accepted, tampered ones get the host mirror's verdict one by one -- the host
and device forms agree, argument errors name the first bad opening, and nothing else on the context is disturbed."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
RAGGED = [1, 2, 3, 5, 255, 256, 257, 1023, 1 << 12, (1 << 15) - 1, (1 << 15) + 1, 1 << 16]
SIZES = [1, 63, 64, 65, 257, 4096, 65537]


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


def _table(seed, n):
    return O.splitmix64_field(seed, n)


def _host_one(o):
    """SimpleMerkleTree::verify (the C++ host mirror) on one opening (root, height, leaf, siblings, dirs)"""
    from zigz_amd import host
    root, h, leaf, sib, dirs = o
    return host.batch_verify([(root, h)], [dict(point=[0] * h, value=0, index=0, leaf=leaf, siblings=sib, directions=dirs)])


def _cols(openings):
    return ([o[0] for o in openings], [o[1] for o in openings], [o[2] for o in openings], [o[3] for o in openings],
            [o[4] for o in openings])


def _host_form(ctx, openings):
    r, h, lv, s, d = _cols(openings)
    return ctx.merkle_verify_batch(b"".join(r), h, lv, b"".join(s), b"".join(d))


def _dev_form(ctx, openings):
    import torch
    r, h, lv, s, d = _cols(openings)
    arrs = [np.frombuffer(b"".join(r) + b"\0" * 32, dtype=np.uint8), np.asarray(lv + [0], dtype=np.uint64),
            np.frombuffer(b"".join(s) + b"\0" * 32, dtype=np.uint8), np.frombuffer(b"".join(d) + b"\0", dtype=np.uint8)]
    ts = [torch.from_numpy(a.copy()).to("cuda") for a in arrs]
    torch.cuda.synchronize()  # (the library runs on its own stream)
    try:
        return ctx.dev_merkle_verify_batch(ts[0].data_ptr(), h, ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr())
    finally:
        del ts


def _both(ctx, openings):
    a, b = _host_form(ctx, openings), _dev_form(ctx, openings)
    assert a.dtype == np.uint8 and len(a) == len(openings)
    assert np.array_equal(a, b)
    return a


def _raw(ctx, openings):
    """the host-form entry called directly: (status, verdicts, n_rejected, bad_index)"""
    from zigz_amd._ffi import lib, u64p, u8p
    r, h, lv, s, d = _cols(openings)
    k = len(openings)
    rb = np.frombuffer(b"".join(r) + b"\0" * 32, dtype=np.uint8).copy()
    sb = np.frombuffer(b"".join(s) + b"\0" * 32, dtype=np.uint8).copy()
    db = np.frombuffer(b"".join(d) + b"\0", dtype=np.uint8).copy()
    la = np.asarray(lv + [0], dtype=np.uint64)
    hs = (C.c_size_t * max(k, 1))(*h)
    verd = np.full(max(k, 1), 0xCD, dtype=np.uint8)
    rej, bad = C.c_size_t(12345), C.c_size_t(99)
    rc = lib.zigz_merkle_verify_batch(ctx.h, k, rb.ctypes.data_as(u8p), hs, la.ctypes.data_as(u64p), sb.ctypes.data_as(u8p),
                                      db.ctypes.data_as(u8p), verd.ctypes.data_as(u8p), C.byref(rej), C.byref(bad))
    return rc, verd[:k], rej.value, bad.value


class Pool:
    """honest openings of the RAGGED tables (padded trees included): the tables committed once, repeated across a batch of
    up to 4096 trees, and opened at random indices as often as needed"""

    def __init__(self, ctx, seed, entries=512):
        self.tables = [_table(seed * 100 + i, n) for i, n in enumerate(RAGGED)]
        self.ns = [RAGGED[i % len(RAGGED)] for i in range(entries)]
        self.res, self.b = ctx.merkle_commit_batch([self.tables[i % len(RAGGED)] for i in range(entries)])
        self.rng = np.random.default_rng(seed)

    def take(self, k):
        out = []
        while len(out) < k:
            idx = [int(self.rng.integers(0, n)) for n in self.ns]
            for (root, h), o in zip(self.res, self.b.open(idx)):
                out.append((root, h, o["value"], o["siblings"], o["directions"]))
        return out[:k]

    def free(self):
        self.b.deinit()


def _flip(b, bit):
    x = bytearray(b)
    x[bit // 8] ^= 1 << (bit % 8)
    return bytes(x)


def _tamper(openings, rng, share=3):
    """a copy of the openings with about 1 / share of them tampered, every kind of tampering in turn"""
    out = list(openings)
    picks = [i for i in range(len(out)) if rng.integers(0, share) == 0]
    for n, i in enumerate(picks):
        root, h, leaf, sib, dirs = out[i]
        kind = n % 8
        if kind == 0:
            leaf ^= 1 << int(rng.integers(0, 64))
        elif kind == 1 and h:
            sib = _flip(sib, 256 * int(rng.integers(0, h)) + int(rng.integers(0, 256)))
        elif kind == 2 and h:
            l = int(rng.integers(0, h))
            dirs = dirs[:l] + bytes([dirs[l] ^ 1]) + dirs[l + 1:]
        elif kind == 3 and h:
            l = int(rng.integers(0, h))
            dirs = dirs[:l] + bytes([(2, 255)[int(rng.integers(0, 2))]]) + dirs[l + 1:]  # != 0 counts as right
        elif kind == 4:
            root = _flip(root, int(rng.integers(0, 256)))
        elif kind == 5 and len(out) > 1:
            j = (i + 1 + int(rng.integers(0, len(out) - 1))) % len(out)
            root, out[j] = out[j][0], (root,) + out[j][1:]  # two openings' roots swapped
        elif kind == 6:
            leaf = leaf + P  # >= p: hashed as given
        else:
            leaf = (leaf + 1) % P
        out[i] = (root, h, leaf, sib, dirs)
    return out


def test_oracle_openings_of_heights_0_to_20_are_accepted(ctx):
    from zigz_amd import host
    rng = np.random.default_rng(1)
    openings, commitments, proofs = [], [], []
    for v in range(21):
        ev = _table(2000 + v, 1 << v)
        root, h = O.merkle_build(ev)
        assert h == v
        pt = [int(x) for x in rng.integers(0, P, size=v)]
        val, idx, sib, dirs, leaf = O.commit_open(P, ev, pt)
        openings.append((root, v, leaf, sib, dirs))
        commitments.append((root, v))
        proofs.append(dict(point=pt, value=val, index=idx, leaf=leaf, siblings=sib, directions=dirs))
    order = list(rng.permutation(21))  # heights mixed in one call
    got = _both(ctx, [openings[i] for i in order])
    assert got.tolist() == [1] * 21
    ok, verd = ctx.commit_verify_batch(commitments, proofs)
    assert ok and verd.tolist() == [1] * 21
    ok, verd = host.batch_verify_dev(ctx, commitments, proofs)  # CommitmentScheme::batchVerify(ctx, ...) of the C++ host
    assert ok and verd.tolist() == [1] * 21
    rc, verd, rej, _ = _raw(ctx, openings)
    assert (rc, verd.tolist(), rej) == (0, [1] * 21, 0)


def test_batched_openings_of_ragged_tables_are_accepted(ctx):
    tables = [_table(3000 + i, n) for i, n in enumerate(RAGGED)]
    res, b = ctx.merkle_commit_batch(tables)
    try:
        n_odd = [n - 1 for n in RAGGED]  # the last real leaf: its sibling is a pad leaf when n is odd
        opened = [b.open(sel) for sel in ([0] * len(RAGGED), n_odd, [n // 2 for n in RAGGED])]
    finally:
        b.deinit()
    openings = [(r, h, o["value"], o["siblings"], o["directions"]) for got in opened for (r, h), o in zip(res, got)]
    assert _both(ctx, openings).tolist() == [1] * len(openings)
    # commit_open_batch over power-of-two tables, checked as CommitmentScheme.batchVerify
    logs = [0, 1, 3, 9, 10, 12, 16]
    pows = [_table(3100 + v, 1 << v) for v in logs]
    pres, pb = ctx.merkle_commit_batch(pows)
    rng = np.random.default_rng(2)
    points = [[int(x) for x in rng.integers(0, P, size=v)] for v in logs]
    try:
        co = ctx.commit_open_batch(pb, points)
    finally:
        pb.deinit()
    proofs = [dict(g, point=pt) for g, pt in zip(co, points)]
    ok, verd = ctx.commit_verify_batch(pres, proofs)
    assert ok and verd.tolist() == [1] * len(logs)


@pytest.mark.parametrize("k", SIZES)
def test_tampered_openings_match_the_host_mirror(ctx, k):
    pool = Pool(ctx, 40 + k)
    try:
        honest = pool.take(k)
    finally:
        pool.free()
    rng = np.random.default_rng(k)
    mixed = _tamper(honest, rng)
    want = np.array([1 if _host_one(o) else 0 for o in mixed], dtype=np.uint8)
    if k >= 63:
        assert 0 < want.sum() < k  # accepts and rejects at random positions
    got = _both(ctx, mixed)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    rc, verd, rej, _ = _raw(ctx, mixed)
    assert rc == 0 and np.array_equal(verd, want) and rej == int((want == 0).sum())


def test_every_kind_of_tampering_on_one_path(ctx):
    ev = _table(4000, 1 << 10)
    root, h = O.merkle_build(ev)
    sib, dirs, leaf = O.merkle_open(ev, 613)
    base = (root, h, leaf, sib, dirs)
    cases = [base, (root, h, leaf ^ 1, sib, dirs), (root, h, leaf + P, sib, dirs), (_flip(root, 0), h, leaf, sib, dirs)]
    for l in range(h):
        cases.append((root, h, leaf, _flip(sib, 256 * l + 7), dirs))
        d = bytearray(dirs)
        d[l] ^= 1
        cases.append((root, h, leaf, sib, bytes(d)))
        for byte in (2, 255):
            d = bytearray(dirs)
            d[l] = byte if dirs[l] else dirs[l]  # a right-hand step written as 2 / 255 is still right
            cases.append((root, h, leaf, sib, bytes(d)))
            d[l] = byte
            cases.append((root, h, leaf, sib, bytes(d)))
    want = [1 if _host_one(o) else 0 for o in cases]
    assert want[0] == 1 and want[1:4] == [0, 0, 0]
    assert _both(ctx, cases).tolist() == want


def test_quirks(ctx):
    from zigz_amd._ffi import lib, u8p, u64p
    # height 0: hashLeaf(value) == root
    one = _table(5000, 1)
    root, h = O.merkle_build(one)
    assert h == 0
    got = _both(ctx, [(root, 0, int(one[0]), b"", b""), (root, 0, int(one[0]) + 1, b"", b""), (root, 0, int(one[0]) + P, b"", b"")])
    assert got.tolist() == [1, 0, 0]
    # k == 0: OK, *n_rejected = 0, nothing else touched
    rc, verd, rej, bad = _raw(ctx, [])
    assert (rc, rej, bad) == (0, 0, 99)
    assert ctx.merkle_verify_batch(b"", [], [], b"", b"").tolist() == []
    ok, verd = ctx.commit_verify_batch([], [])
    assert ok and len(verd) == 0
    # the index and the point's values are not part of the Merkle check; a point of the wrong length rejects that opening only
    logs = [4, 6, 8]
    tables = [_table(5100 + v, 1 << v) for v in logs]
    res, b = ctx.merkle_commit_batch(tables)
    try:
        pts = [[1] * v for v in logs]
        co = ctx.commit_open_batch(b, pts)
    finally:
        b.deinit()
    proofs = [dict(g, point=pt) for g, pt in zip(co, pts)]
    moved = [dict(p, index=p["index"] + 5, point=[7] * len(p["point"]), value=(p["value"] + 1) % P) for p in proofs]
    assert ctx.commit_verify_batch(res, moved)[1].tolist() == [1, 1, 1]
    short = [dict(p) for p in proofs]
    short[1]["point"] = short[1]["point"][:-1]
    ok, verd = ctx.commit_verify_batch(res, short)
    assert not ok and verd.tolist() == [1, 0, 1]
    assert ctx.commit_verify_batch(res, proofs[:2]) == (False, None)
    # k above the maximum is refused before anything runs
    z = np.zeros(64, dtype=np.uint64)
    zp, zb = z.ctypes.data_as(u64p), z.ctypes.data_as(u8p)
    assert lib.zigz_merkle_verify_batch(ctx.h, (1 << 22) + 1, zb, (C.c_size_t * 1)(0), zp, zb, zb, None, C.byref(C.c_size_t()),
                                        None) == E.INVALID_ARGUMENT  # (refused before heights[1..] would be read)


def test_argument_errors_name_the_first_bad_opening(ctx):
    from zigz_amd._ffi import lib, u8p, u64p
    pool = Pool(ctx, 7, entries=16)
    try:
        ops = pool.take(6)
    finally:
        pool.free()
    rc, verd, rej, bad = _raw(ctx, ops)
    assert rc == 0 and verd.tolist() == [1] * 6
    r, h, lv, s, d = _cols(ops)
    # a height above 64 -- at index 4 (and at 5): the first one is named, nothing runs, the outputs stay as they were
    hs = list(h)
    hs[4] = hs[5] = 65
    rb = np.frombuffer(b"".join(r), dtype=np.uint8).copy()
    sb = np.frombuffer(b"".join(s) + b"\0" * (32 * 130), dtype=np.uint8).copy()
    db = np.frombuffer(b"".join(d) + b"\0" * 130, dtype=np.uint8).copy()
    la = np.asarray(lv, dtype=np.uint64)
    verd = np.full(6, 0xCD, dtype=np.uint8)
    rej, badi = C.c_size_t(777), C.c_size_t(99)
    args = [rb.ctypes.data_as(u8p), (C.c_size_t * 6)(*hs), la.ctypes.data_as(u64p), sb.ctypes.data_as(u8p), db.ctypes.data_as(u8p),
            verd.ctypes.data_as(u8p), C.byref(rej), C.byref(badi)]
    assert lib.zigz_merkle_verify_batch(ctx.h, 6, *args) == E.INVALID_ARGUMENT
    assert (badi.value, rej.value) == (4, 777) and (verd == 0xCD).all()
    with pytest.raises(E.ZigzError) as e:
        ctx.merkle_verify_batch(b"".join(r), hs, lv, bytes(sb[: 32 * sum(hs)]), bytes(db[: sum(hs)]))
    assert (e.value.code, e.value.bad_index) == (E.INVALID_ARGUMENT, 4)
    # NULL arrays when k > 0, a NULL context, a NULL n_rejected
    good = [rb.ctypes.data_as(u8p), (C.c_size_t * 6)(*h), la.ctypes.data_as(u64p), sb.ctypes.data_as(u8p), db.ctypes.data_as(u8p)]
    for i in range(5):
        a = list(good)
        a[i] = None
        assert lib.zigz_merkle_verify_batch(ctx.h, 6, *a, None, C.byref(rej), None) == E.INVALID_ARGUMENT, i
    assert lib.zigz_merkle_verify_batch(None, 6, *good, None, C.byref(rej), None) == E.INVALID_ARGUMENT
    assert lib.zigz_merkle_verify_batch(ctx.h, 6, *good, None, None, None) == E.INVALID_ARGUMENT
    # verdicts may be NULL: the count alone
    rej.value = 777
    assert lib.zigz_merkle_verify_batch(ctx.h, 6, *good, None, C.byref(rej), None) == 0 and rej.value == 0
    # the device form refuses misaligned roots / siblings / values
    import torch
    t = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(E.ZigzError) as e:
        ctx.dev_merkle_verify_batch(t.data_ptr() + 4, [1], t.data_ptr() + 256, t.data_ptr() + 512, t.data_ptr() + 768)
    assert e.value.code == E.INVALID_ARGUMENT
    # the context still works
    assert _both(ctx, ops).tolist() == [1] * 6


def test_at_scale_2_18_openings_of_height_20(ctx):
    """2^18 openings of one 2^20 table (a device batch of 64 entries that repeat it, opened 4096 times), a known random
    subset tampered: every verdict as expected, a sample cross-checked with the host mirror.  The host form runs in chunks."""
    n, entries, k = 1 << 20, 64, 1 << 18
    t = _table(6000, n)
    import torch
    dt = torch.from_numpy(t.astype(np.uint32).view(np.int32)).to("cuda")  # packed u32
    torch.cuda.synchronize()
    res, b = ctx.dev_merkle_commit_batch([dt.data_ptr()] * entries, [n] * entries)
    rng = np.random.default_rng(18)
    try:
        assert res[0] == O.merkle_build(t) and all(r == res[0] for r in res)
        root = res[0][0]
        sibs, dirs, leaves = [], [], []
        for _ in range(k // entries):
            for o in b.open([int(x) for x in rng.integers(0, n, size=entries)]):
                sibs.append(o["siblings"])
                dirs.append(o["directions"])
                leaves.append(o["value"])
    finally:
        b.deinit()
        del dt
    bad = rng.random(k) < 0.01
    roots = [root] * k
    for i in np.nonzero(bad)[0]:
        if i % 2:
            sibs[i] = _flip(sibs[i], int(rng.integers(0, 20 * 256)))
        else:
            leaves[i] = (leaves[i] + 1) % P
    openings = [(roots[i], 20, leaves[i], sibs[i], dirs[i]) for i in range(k)]
    want = (~bad).astype(np.uint8)
    got = _both(ctx, openings)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    for i in list(rng.choice(k, size=200, replace=False)) + list(np.nonzero(bad)[0][:50]):
        assert int(got[i]) == (1 if _host_one(openings[i]) else 0), i


def test_verify_behind_an_active_commit_job(ctx):
    import zigz_amd
    nv = 11
    cols = np.stack([O.splitmix64_field(7000 + c, 1 << nv) for c in range(43)])
    cexp = O.generate_commitments(P, O.Transcript(), cols, fast=True)
    pool = Pool(ctx, 71, entries=64)
    try:
        ops = _tamper(pool.take(3000), np.random.default_rng(71))
    finally:
        pool.free()
    want = np.array([1 if _host_one(o) else 0 for o in ops], dtype=np.uint8)
    job = zigz_amd.CommitJob(ctx, cols=cols)
    try:
        v1 = _host_form(ctx, ops)  # queued behind the job's build
        roots = job.roots()
        before = ctx.stats()
        v2 = _dev_form(ctx, ops)
        after = ctx.stats()
        opened = job.open_all(cexp["points"])
    finally:
        job.end()
    assert before == after
    assert np.array_equal(roots, cexp["roots"])
    for key in ("values", "indices", "leaves", "siblings", "dirs"):
        assert np.array_equal(opened[key], cexp[key]), key
    assert np.array_equal(v1, want) and np.array_equal(v2, want)


def test_two_contexts_verify_while_a_third_commits(ctx):
    import zigz_amd
    pool = Pool(ctx, 81, entries=128)
    try:
        sets = [_tamper(pool.take(5000), np.random.default_rng(81 + c)) for c in range(2)]
    finally:
        pool.free()
    wants = [np.array([1 if _host_one(o) else 0 for o in s], dtype=np.uint8) for s in sets]
    nv = 11
    cols = np.stack([O.splitmix64_field(8000 + c, 1 << nv) for c in range(43)])
    cexp = O.generate_commitments(P, O.Transcript(), cols, fast=True)
    out, errs = [None, None, None], []

    def verify(c):
        try:
            cx = zigz_amd.Context(0)
            out[c] = [(_host_form(cx, sets[c]), _dev_form(cx, sets[c])) for _ in range(3)]
            cx.close()
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    def commit():
        try:
            cx = zigz_amd.Context(0)
            got = []
            for _ in range(3):
                job = zigz_amd.CommitJob(cx, cols=cols)
                try:
                    got.append((job.roots(), job.open_all(cexp["points"])))
                finally:
                    job.end()
            out[2] = got
            cx.close()
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    th = [threading.Thread(target=verify, args=(c,)) for c in range(2)] + [threading.Thread(target=commit)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for c in range(2):
        for a, b in out[c]:
            assert np.array_equal(a, wants[c]) and np.array_equal(b, wants[c])
    for roots, opened in out[2]:
        assert np.array_equal(roots, cexp["roots"])
        for key in ("values", "indices", "leaves", "siblings", "dirs"):
            assert np.array_equal(opened[key], cexp[key]), key
