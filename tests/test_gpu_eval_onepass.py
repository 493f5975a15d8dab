"""The opening evaluation of a commit job in one launch (kernels.hip: k_eval_onepass), finished inside the paths launch (k_paths
adds a column's partials, reduces mod p and stores the value).  All arithmetic is exact mod p, so every opened value must be the
canonical u32 of tests/exact_ref.py's eval and of the same job evaluated by v successive binds (option fold_eval).

Shapes: nv 14 (one row group of 16 rows, no lists below 2^15: nothing skipped), 15 (32 rows), 17 (two groups of 64), 20 (16
groups); 1, 2, 43 and 70 columns (above 64 columns nothing is list-built and nothing skipped).  Within a job the columns take
turns at the kinds of point, so one build covers them all."""
import numpy as np
import pytest

import exact_ref
import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
ALL = (1 << 62) - 1
OFF = {"small_domain_mask": 0, "run_aware_mask": 0, "cons_group_mask": 0, "fold_eval": 0}
POINT_KINDS = 5


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


def _points(nv, ncols, seed):
    """column c takes kind (c + seed) % 5: random, all 0, all 1, all p - 1, random with one coordinate p - 1"""
    pts = O.splitmix64_field(1000 + seed, ncols * nv).reshape(ncols, nv).copy()
    for c in range(ncols):
        kind = (c + seed) % POINT_KINDS
        if kind == 1:
            pts[c, :] = 0
        elif kind == 2:
            pts[c, :] = 1
        elif kind == 3:
            pts[c, :] = P - 1
        elif kind == 4:
            pts[c, (c * 7 + seed) % nv] = P - 1
    return pts


def _random_table(nv, ncols, seed):
    return np.random.default_rng(seed).integers(0, P, size=(ncols, 1 << nv), dtype=np.uint64)


def _columns(base, constant):
    """a copy of the table `base` in which `constant` columns (spread over the job) hold one value each -- the first of them
    p - 1 -- and the last of the others is all p - 1 but for one entry.  Returns (columns, which are constant, that last column
    or -1)."""
    ncols, N = base.shape
    cols = base.copy()
    is_const = np.zeros(ncols, dtype=bool)
    if constant:
        is_const[np.linspace(0, ncols - 1, constant).round().astype(int)] = True
    first = True
    for c in np.flatnonzero(is_const):
        cols[c, :] = P - 1 if first else (c * 1000003 + 5) % P
        first = False
    busy = np.flatnonzero(~is_const)
    last = int(busy[-1]) if busy.size else -1
    if last >= 0:
        cols[last, :] = P - 1
        cols[last, N // 3] = P - 2
    return cols, is_const, last


def _open(ctx, d, ncols, nv, pts, opts):
    import zigz_amd
    saved = _options(ctx, dict(OFF, **opts))
    try:
        job = zigz_amd.CommitJob(ctx, d_cols=d, ncols=ncols, nv=nv, col_stride=1 << nv)
        try:
            job.roots()
            o = {k: v.copy() for k, v in job.open_all(pts).items()}
            st = ctx.stats()
        finally:
            job.end()
    finally:
        _options(ctx, saved)
    return o, st


def _upload(ctx, cols):
    d = ctx.dev_alloc(cols.size * 4)
    ctx.upload(cols.reshape(-1), d)
    return d


def _constant_counts(nv, ncols):
    """zero, one, most and all columns constant -- where a constant column can be skipped at all (lists from 2^15 leaves, up to
    64 columns); elsewhere the pattern changes no path: none and most"""
    if nv < 15 or ncols > 64:
        return sorted({0, ncols - 1})
    return sorted({0, 1, ncols - 1, ncols})


@pytest.mark.parametrize("ncols", [1, 2, 43, 70])
@pytest.mark.parametrize("nv", [14, 15, 17, 20])
def test_values_equal_the_exact_evaluation(ctx, nv, ncols):
    """every kind of point; run-aware hints on (constant columns are skipped where the build has lists) and off; against
    exact_ref.eval (computed once per column of the random table) and against the same job evaluated by v successive binds"""
    base = _random_table(nv, ncols, 31 * nv + ncols)
    pts = _points(nv, ncols, nv + ncols)
    exact = [exact_ref.eval(base[c], pts[c]) for c in range(ncols)]
    for constant in _constant_counts(nv, ncols):
        cols, is_const, last = _columns(base, constant)
        want = np.array([int(cols[c, 0]) if is_const[c] else exact[c] for c in range(ncols)], dtype=np.uint64)
        if last >= 0:
            want[last] = exact_ref.eval(cols[last], pts[last])
        d = _upload(ctx, cols)
        try:
            hinted, st = _open(ctx, d, ncols, nv, pts, {"run_aware_mask": ALL})
            plain, _ = _open(ctx, d, ncols, nv, pts, {})
            folds, _ = _open(ctx, d, ncols, nv, pts, {"run_aware_mask": ALL, "fold_eval": 1})
        finally:
            ctx.dev_free(d)
        if 15 <= nv and ncols <= 64:
            assert st["eval_constant_columns"] == constant
        for name, o in (("hinted", hinted), ("plain", plain), ("folds", folds)):
            bad = np.flatnonzero(o["values"] != want)
            assert bad.size == 0, (name, constant, "column", int(bad[0]), int(o["values"][bad[0]]), int(want[bad[0]]))
        for k in hinted:
            assert np.array_equal(hinted[k], folds[k]) and np.array_equal(hinted[k], plain[k]), k


def test_no_eval_skip_job(ctx):
    """a job that must not skip (measurement mode debug_skip = 2 sets no_eval_skip): constant columns go through the fold"""
    nv, ncols = 16, 43
    cols, _, _ = _columns(_random_table(nv, ncols, 5), 40)
    d = _upload(ctx, cols)
    try:
        pts = _points(nv, ncols, 2)
        want = np.array([exact_ref.eval(cols[c], pts[c]) for c in range(ncols)], dtype=np.uint64)
        first, _ = _open(ctx, d, ncols, nv, pts, {"run_aware_mask": ALL})  # (leaves the lists the skipped passes would write)
        ctx.set_option("debug_skip", 2)
        try:
            o, _ = _open(ctx, d, ncols, nv, pts, {"run_aware_mask": ALL})
        finally:
            ctx.set_option("debug_skip", 0)
        assert np.array_equal(first["values"], want)
        assert np.array_equal(o["values"], want)
    finally:
        ctx.dev_free(d)


def test_arena_batch_of_three(ctx):
    """three proofs of 43 columns in one batched job at 2^15 (columns numbered proof by proof, one arena each)"""
    import zigz_amd
    nv, ncols = 15, 43
    sets = [_columns(_random_table(nv, ncols, 70 + k), k)[:2] for k in (0, 41, 43)]
    bufs = [_upload(ctx, cols) for cols, _ in sets]
    pts = np.concatenate([_points(nv, ncols, z) for z in range(3)])
    want = np.array([int(cols[c, 0]) if is_const[c] else exact_ref.eval(cols[c], pts[z * ncols + c])
                     for z, (cols, is_const) in enumerate(sets) for c in range(ncols)], dtype=np.uint64)
    saved = _options(ctx, dict(OFF, run_aware_mask=(1 << 43) - 1))
    try:
        job = zigz_amd.CommitJob(ctx, d_cols_list=bufs, ncols=ncols, nv=nv, col_stride=1 << nv)
        try:
            job.roots()
            o = job.open_all(pts)
            got = o["values"].copy()
            leaves = o["leaves"].copy()
        finally:
            job.end()
    finally:
        _options(ctx, saved)
        for d in bufs:
            ctx.dev_free(d)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("column", int(bad[0]))
    for z, (cols, _) in enumerate(sets):
        for c in range(ncols):
            assert int(leaves[z * ncols + c]) == int(cols[c, int(pts[z * ncols + c, 0]) % (1 << nv)])
