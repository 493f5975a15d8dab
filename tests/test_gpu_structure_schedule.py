"""The fused structure schedule (merkle_levels.hip): the table passes of the levels >= 1 and the runs stages >= 2 ride in the
level-hash launches, the rest of the structure work in two launches (A, B) plus the keep / drop decision.  Whatever the
schedule, a structure-aware build must give the dense build's trees: roots, opened paths and evaluations, node for node where
the trees are materialised."""
import numpy as np
import pytest

import oracle_lib as O
import programs

pytestmark = pytest.mark.gpu

SMALL = (1 << 1) | (0x3f << 33) | (1 << 42)
HINTS = {"small_domain_mask": SMALL, "run_aware_mask": (0x7fffffff << 2) | (3 << 40),
         "cons_group_mask": 1 | (1 << 1) | (0x7f << 33) | (1 << 42)}
DENSE = {k: 0 for k in HINTS}


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    c = zigz_amd.Context(0)
    yield c
    c.close()


def _options(ctx, opts):
    saved = {k: ctx.get_option(k) for k in opts}
    for k, v in opts.items():
        ctx.set_option(k, v)
    return saved


def _trace(ctx, prog):
    """resident witness columns of a program's trace -> (device pointer, padded rows)"""
    from zigz_amd import host
    tr = host.Trace(prog, 0x1000, None, 1 << 21)
    N = 1 << tr.num_vars
    d = ctx.dev_alloc(43 * N * 4)
    tr.witness_to_device(ctx, d, N)
    return d, tr.num_vars


def _job(ctx, d, nv, opts, pts, d_list=None):
    """(roots, openings, stats) of one commit job under the given options"""
    import zigz_amd
    saved = _options(ctx, opts)
    try:
        if d_list is not None:
            job = zigz_amd.CommitJob(ctx, d_cols_list=d_list, ncols=43, nv=nv, col_stride=1 << nv)
        else:
            job = zigz_amd.CommitJob(ctx, d_cols=d, ncols=43, nv=nv, col_stride=1 << nv)
        try:
            roots = job.roots().copy()
            st = ctx.stats()
            outs = {k: v.copy() for k, v in job.open_all(pts).items()}
        finally:
            job.end()
    finally:
        _options(ctx, saved)
    return roots, outs, st


def _points(nv, n, seed):
    pts = np.random.default_rng(seed).integers(0, O.P_BB, size=(n, nv), dtype=np.uint64)
    pts[:, 0] = np.random.default_rng(seed + 1).integers(0, 1 << nv, size=n)  # (the opened index rides in the point)
    return pts


def _same(a, b):
    ra, oa = a[0], a[1]
    rb, ob = b[0], b[1]
    assert np.array_equal(ra, rb)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k


def _prog(kind, N):
    if kind == "add_xor":
        return programs.add_xor_loop((N - 3) // 4)
    if kind == "mixed":
        return programs.mixed_loop((N - 8) // 12 - 3)
    if kind == "round_robin":
        return programs.register_round_robin((N - 2) // 31 - 1)
    return programs.straight_line_program(7, int(0.9 * N))  # never repeats: the group is dropped


@pytest.mark.parametrize("nv", [16, 20])
@pytest.mark.parametrize("kind", ["add_xor", "mixed", "round_robin", "straight"])
def test_traces_equal_the_dense_build(ctx, kind, nv):
    """The bench trace, the RV64IM mix (config 4's loop), the worst-case register trace and a straight-line program (its
    group dropped on the device): roots, paths and evaluations equal the dense build's -- three jobs in a row, so that the
    context's later builds leave the probe out (two kept groups) where the group repeats."""
    d, got_nv = _trace(ctx, _prog(kind, 1 << nv))
    assert got_nv == nv
    pts = _points(nv, 43, nv * 7 + len(kind))
    ref = _job(ctx, d, nv, DENSE, pts)
    saved = _options(ctx, {"cons_always": 1})
    try:
        for _ in range(3):
            r = _job(ctx, d, nv, HINTS, pts)
            _same(ref, r)
    finally:
        _options(ctx, saved)
    st = r[2]
    if kind == "straight":
        assert st["cons_columns"] == 0
    else:
        assert st["cons_columns"] == 10 and st["cons_hashed"] < st["cons_dense_nodes"]
    assert st["run_aware_columns"] > 0
    ctx.dev_free(d)


def test_probe_on_and_left_out(ctx):
    """The probe in front of A, and left out once the context's last two builds kept their group: same trees either way."""
    nv = 18
    d, _ = _trace(ctx, _prog("mixed", 1 << nv))
    pts = _points(nv, 43, 5)
    ref = _job(ctx, d, nv, DENSE, pts)
    seen = []
    for _ in range(4):
        r = _job(ctx, d, nv, HINTS, pts)
        _same(ref, r)
        seen.append(r[2]["cons_probe_distinct"])
    assert seen[0] > 0          # the first build probes (the count is the probe's sample)
    assert r[2]["cons_columns"] == 10
    ctx.dev_free(d)


@pytest.mark.parametrize("kind,n", [("straight", (1 << 15) - 1), ("straight", (1 << 15) + 1), ("add_xor", 8191), ("add_xor", 8192)])
def test_padded_sizes_around_2p15(ctx, kind, n):
    """Traces just under and over 2^15 steps (2^15 and 2^16 padded rows: the smallest list-built trees, and the first size
    with a probe): a straight-line program of 2^15 - 1 / 2^15 + 1 steps (its group dropped) and the bench loop with 2^15 - 1 /
    2^15 + 3 steps (kept)."""
    prog = programs.straight_line_program(11, n) if kind == "straight" else programs.add_xor_loop(n)
    d, nv = _trace(ctx, prog)
    assert nv == (15 if n in ((1 << 15) - 1, 8191) else 16)
    pts = _points(nv, 43, n)
    ref = _job(ctx, d, nv, DENSE, pts)
    saved = _options(ctx, {"cons_always": 1})
    try:
        for _ in range(3):
            _same(ref, _job(ctx, d, nv, HINTS, pts))
    finally:
        _options(ctx, saved)
    ctx.dev_free(d)


def _tree_words(ctx, job, ncols):
    d, per_col = job.tree()
    return ctx.download(d, ncols * per_col // 4).astype(np.uint32)


@pytest.mark.parametrize("nv", [16, 17])
def test_one_column_group_whole_trees(ctx, nv):
    """A group of ONE column (next to a run-aware column and a group of three): every node of every materialised tree equals
    the dense build's."""
    import zigz_amd
    N = 1 << nv
    nc = 6
    step = np.arange(N)
    cols = O.splitmix64_field(700 + nv, nc * N).reshape(nc, N).copy()
    cols[0, :] = 0x1000 + 4 * (step % 12)
    cols[1, :] = np.repeat(O.splitmix64_field(3, N // 64), 64)
    cols[2, :] = (step % 12) % 5
    cols[3, :] = step % 7
    trees = []
    for g, r in ((0, 0), (1 << 0, 1 << 1), (1 << 3, 1 << 1), ((1 << 0) | (1 << 2) | (1 << 3), 1 << 1)):
        saved = _options(ctx, {"cons_group_mask": g, "run_aware_mask": r, "run_aware_materialize": 1})
        try:
            job = zigz_amd.CommitJob(ctx, cols=cols)
            try:
                trees.append((job.roots().copy(), _tree_words(ctx, job, nc), ctx.stats()))
            finally:
                job.end()
        finally:
            _options(ctx, saved)
    r0, t0, _ = trees[0]
    for r, t, st in trees[1:]:
        assert np.array_equal(r, r0)
        bad = np.nonzero(t != t0)[0]
        assert bad.size == 0, ("first differing node", int(bad[0]) // 8)
    assert trees[1][2]["cons_columns"] == 1 and trees[2][2]["cons_columns"] == 1


def test_arena_batch_equals_dense_single_jobs(ctx):
    """Several proofs in one commit job (gridDim.z = proof): each proof's roots and openings equal its own dense job's."""
    nv = 18
    N = 1 << nv
    kinds = ["add_xor", "mixed", "straight", "round_robin"]
    bufs = [_trace(ctx, _prog(k, N))[0] for k in kinds]
    pts = [_points(nv, 43, 40 + i) for i in range(len(kinds))]
    single = [_job(ctx, d, nv, DENSE, p) for d, p in zip(bufs, pts)]
    saved = _options(ctx, {"cons_always": 1})
    try:
        r, o, _ = _job(ctx, None, nv, HINTS, np.concatenate(pts), d_list=bufs)
    finally:
        _options(ctx, saved)
    for z, (rs, os_, _) in enumerate(single):
        assert np.array_equal(r[z * 43:(z + 1) * 43], rs), kinds[z]
        for k in ("values", "indices", "leaves", "siblings", "dirs"):
            assert np.array_equal(o[k][z * 43:(z + 1) * 43], os_[k]), (kinds[z], k)
    for d in bufs:
        ctx.dev_free(d)


def test_hinted_build_after_a_different_trace_is_rebuilt(ctx):
    """Lists sized by what the context's earlier builds needed: after the bench trace (few hashed nodes), the worst-case
    register trace outgrows them, the build is repeated with more room -- and still equals the dense build."""
    nv = 18
    N = 1 << nv
    d0, _ = _trace(ctx, _prog("add_xor", N))
    d1, _ = _trace(ctx, _prog("round_robin", N))
    pts = _points(nv, 43, 77)
    ref = _job(ctx, d1, nv, DENSE, pts)
    for _ in range(3):
        _job(ctx, d0, nv, HINTS, pts)
    before = ctx.stats()["rebuilds"]
    r = _job(ctx, d1, nv, HINTS, pts)
    _same(ref, r)
    assert ctx.stats()["rebuilds"] > before
    _same(ref, _job(ctx, d1, nv, HINTS, pts))


def test_measurement_mode_without_hashing_still_runs_every_pass(ctx):
    """Option debug_skip = 1 (no hash launches; the separate schedule): the structure passes all run, so a trace that outgrows
    the room learnt from another is found out -- and repeated -- exactly as in a normal build, and the probe counts the same."""
    nv = 18
    N = 1 << nv
    d0, _ = _trace(ctx, _prog("add_xor", N))
    d1, _ = _trace(ctx, _prog("round_robin", N))
    pts = _points(nv, 43, 78)

    def learn_then_switch(skip):
        import zigz_amd
        c = zigz_amd.Context(0)
        try:
            for _ in range(3):
                _job(c, d0, nv, HINTS, pts)
            c.set_option("debug_skip", skip)
            try:
                before = c.stats()["rebuilds"]
                _, _, st = _job(c, d1, nv, HINTS, pts)
                return c.stats()["rebuilds"] - before, st["cons_probe_distinct"], st["run_aware_columns"]
            finally:
                c.set_option("debug_skip", 0)
        finally:
            c.close()

    normal = learn_then_switch(0)
    skipped = learn_then_switch(1)
    assert normal[0] >= 1
    assert skipped == normal
