"""Structure-aware Merkle builds at 2^21 .. 2^27 leaves against an exact host reference (tests/merkle_ref.py: numpy + hashlib,
pinned to the C oracle by tests/test_merkle_ref_cpu.py) -- column by column: every root, opening paths at the indices next to
every boundary of the schedule, the opened values, and the counters that say WHICH path built the trees.

What is new at these sizes (merkle_levels.hip, build_trees in api_commit.cpp):
  2^21 ..  H(0) carries the table pass of level 1, runs stage 2 and the leaf hashes (k_level_hash_rides<true, true, true>);
           the levels 13 .. of the run-aware lists exist only through that riding stage
  2^24     stage 2 has exactly one full segment            2^25  two segments per column; the last size of the group path
  2^26     RUN_MAX_LEAVES: four segments, the group hint is given but not taken
  2^27     above the limit: run-aware and group hints are ignored, the small-domain hint still applies
All builds are commit jobs on the default schedule with virtual copies.  The reference of a column set is computed once per
module.  Every test prints how its time splits into reference and GPU work (pytest -s).

Opened values: the FIRST build of a set opens every column at a random point and compares with the full multilinear eval
(exact_ref.eval) -- one random point per column and set, also at 2^25 and 2^26; the other ~21 builds of the set use points whose
coordinates 1 .. are the opened index's bits, where the value is the line a + idx * (b - a) through two neighbouring leaves:
exact, and it keeps a 2^26 fold per column and build out of the suite."""
import os
import time

import numpy as np
import pytest

import exact_ref
import merkle_ref as M
import oracle_lib as O
import programs

pytestmark = pytest.mark.gpu

P = O.P_BB
_FULL = pytest.mark.skipif(os.environ.get("ZIGZ_TEST_SKIP_FULL") == "1", reason="2^26 and 2^27 runs skipped by request")
# (size, steps of the group's loop).  8191 = 2^13 - 1: never aligned, the group's lists are long at every level -- run where the
# group path exists (up to 2^25; at 2^26 the group's columns are dense / small-domain columns whatever they hold)
MIXED = [(nv, period) for nv in (21, 22, 23, 24, 25) for period in (12, 8191)] + [pytest.param(26, 12, marks=_FULL)]
TAIL = 1000  # the last leaves of the group columns break the loop (a padded trace)


def rnd(seed, n):
    return O.splitmix64_field(seed, n)


# ---------------------------------------------------------------- which path a column must take (the limits stated in kernels.hpp / build_trees)
def _kinds(nv, ncols, hints):
    """(G, H, R): the columns a commit job builds content-addressed, from the small-domain tables, run-aware; the rest densely.
    RUN_MIN_LEAVES = 2^15 <= npad <= RUN_MAX_LEAVES = 2^26 for lists at all, the group one size less; tables from 2^10."""
    big = 15 <= nv <= 26 and ncols <= 64
    cons, sd, run = hints["cons_group_mask"], hints["small_domain_mask"], hints["run_aware_mask"]
    G = [c for c in range(ncols) if big and nv < 26 and (cons >> c) & 1]
    H = [c for c in range(ncols) if c not in G and nv >= 10 and (sd >> c) & 1]
    R = [c for c in range(ncols) if c not in G and c not in H and big and (run >> c) & 1]
    return G, H, R


# ---------------------------------------------------------------- column sets
GROUP = [0, 1, 2, 3, 4]
RUNS = [5, 6, 7, 8, 9, 10]
HINTS = {"cons_group_mask": sum(1 << c for c in GROUP),
         "small_domain_mask": (1 << 1) | (1 << 3) | (1 << 11),
         "run_aware_mask": sum(1 << c for c in RUNS) | (1 << 11)}
NCOLS = 13


def _boundaries(nv):
    """the leaf positions next to which builds go wrong: the chunk of 64, the stage-0 segment, the stage-1 segment (2^18 leaves),
    the stage-2 segment (2^24 leaves, where the size has more than one), the middle"""
    N = 1 << nv
    return sorted({64, 4096, 1 << 18, N // 2} | ({1 << 24} if nv > 24 else set()))


def _group_columns(nv, period):
    N = 1 << nv
    step = np.arange(N, dtype=np.int64)
    ph = step % period
    cols = [0x1000 + 4 * ph,                         # "pc": a loop of `period` steps
            ph % 5,                                  # a function of it (small-domain)
            ph * 1000003 % P,                        # another
            np.zeros(N, dtype=np.int64),             # constant (x0)
            np.where(ph == 3, 1, 0)]
    cols[0][N - TAIL:] = 0x1000 + 4 * (period - 1)   # the padding of a trace: pc repeats its last value ...
    for c in (1, 2, 4):
        cols[c][N - TAIL:] = 0                       # ... while the instruction fields drop to 0
    return [c.astype(np.uint32) for c in cols]


def _other_columns(nv):
    N = 1 << nv
    step = np.arange(N, dtype=np.int64)
    seg2 = min(1 << 24, N // 2)                      # one stage-2 segment of leaves where the size has several
    changes = sorted(set(b + d for b in _boundaries(nv) for d in (-1, 0, 1)) | {N - 1})
    cols = [np.full(N, 5),                                                   # 5  constant
            np.zeros(N, dtype=np.int64),                                     # 6  all zero
            np.repeat(rnd(1, N // 1000 + 1), 1000)[:N],                      # 7  runs of 1000: boundaries anywhere
            np.repeat(rnd(2, N // seg2), seg2),                              # 8  aligned runs of one stage-2 segment
            1 + np.searchsorted(np.array(changes), step, side="right"),      # 9  single changes next to every boundary
            np.repeat(rnd(3, 7)[np.arange(N // 3 + 1) % 7], 3)[:N],          # 10 runs of 3 over a cycle of 7 values
            np.repeat(np.arange(N // 512) % 128, 512),                       # 11 small-domain AND piecewise constant
            rnd(4, 509)[step % 509]]                                         # 12 unhinted, looks random: built densely
    return [np.asarray(c).astype(np.uint32) for c in cols]


class _Set:
    """columns (u32), their references, the group's and the run-aware model's counts, and what computing them cost"""

    def __init__(self, cols, hints, nv):
        self.cols, self.hints, self.nv = cols, hints, nv
        self.G, self.H, self.R = _kinds(nv, len(cols), hints)
        self.refs, self.group, self.run_hashed, self.ref_s = [None] * len(cols), None, 0, 0.0

    def finish(self):
        t0 = time.perf_counter()
        for c, col in enumerate(self.cols):
            if self.refs[c] is None:
                self.refs[c] = M.MerkleRef(col)
        levels = M._list_levels(self.nv)
        if self.G:
            g = M.GroupRef([self.cols[c] for c in self.G])
            self.group = sum(g.distinct_tuples(l) for l in range(levels))
        if self.R:
            self.run_hashed = M._run_aware_hashed([self.cols[c] for c in self.R], levels)
        self.ref_s += time.perf_counter() - t0
        self.hashes = sum(r.hashes for r in self.refs)
        return self


_CACHE = {}


def _evict(nv):
    """lets the large sets of other sizes go (2^26: several GB of columns and ids)"""
    for k in [k for k in _CACHE if k[0] != nv and k[0] >= 24]:
        del _CACHE[k]


def _set(nv, period):
    """the column set of a size with a group loop of `period` steps: computed once, the columns outside the group (and their
    references) shared between the periods"""
    _evict(nv)
    if (nv, period) not in _CACHE:
        if (nv, 0) not in _CACHE:
            t0 = time.perf_counter()
            other = _other_columns(nv)
            _CACHE[nv, 0] = (other, [M.MerkleRef(c) for c in other], time.perf_counter() - t0)
        other, other_refs, other_s = _CACHE[nv, 0]
        s = _Set(_group_columns(nv, period) + other, HINTS, nv)
        s.refs[len(GROUP):] = other_refs
        s.ref_s = other_s
        _CACHE[nv, period] = s.finish()
    return _CACHE[nv, period]


# ---------------------------------------------------------------- builds
@pytest.fixture()
def ctx():
    import zigz_amd
    c = zigz_amd.Context(0)
    yield c
    c.close()


def _hint(ctx, hints):
    for k, v in hints.items():
        ctx.set_option(k, v)


def _upload(ctx, cols):
    N = cols[0].size
    d = ctx.dev_alloc(len(cols) * N * 4)
    for c, col in enumerate(cols):
        ctx.upload(col.astype(np.uint64), d + c * N * 4)
    return d


def _points(nv, idx, seed, boolean):
    """one point per column; the opened index rides in coordinate 0.  boolean: the other coordinates are the index's bits, so
    that the value is a line through two neighbouring leaves (checked without a 2^nv fold)."""
    nc = len(idx)
    pts = rnd(seed, nc * nv).reshape(nc, nv).copy()
    if boolean:
        for c in range(nc):
            pts[c, 1:] = [(int(idx[c]) >> k) & 1 for k in range(1, nv)]
    pts[:, 0] = idx
    return pts


def _build(ctx, d, ncols, nv, pts):
    import zigz_amd
    job = zigz_amd.CommitJob(ctx, d_cols=d, ncols=ncols, nv=nv, col_stride=1 << nv)
    try:
        roots = job.roots().copy()
        st = ctx.stats()
        o = {k: v.copy() for k, v in job.open_all(pts).items()}
    finally:
        job.end()
    return roots, o, st


def _check_stats(s, st):
    """the path was really taken: a build that fell back to the dense kernels fails here"""
    N, levels = 1 << s.nv, M._list_levels(s.nv)
    assert st["run_aware_columns"] == len(s.R)
    assert st["cons_columns"] == len(s.G), {k: st[k] for k in ("cons_columns", "cons_probe_distinct", "cons_hashed", "rebuilds")}
    assert st["small_domain_columns"] == len(s.H)
    assert st["run_aware_hashed"] == s.run_hashed
    assert st["run_aware_dense_nodes"] == len(s.R) * sum(N >> l for l in range(levels)) * (1 if s.R else 0)
    # a kept group hashes, per column, one node per distinct tuple of subtrees on every list level
    assert st["cons_hashed"] == (len(s.G) * s.group if s.G else 0)


def _check(s, roots, o, pts, boolean):
    nv = s.nv
    for c, ref in enumerate(s.refs):
        assert roots[c].tobytes() == ref.root, ("root of column", c)
    for c, ref in enumerate(s.refs):
        i = int(pts[c, 0])
        sib, dirs, leaf = ref.open(i)
        where = (c, i)
        assert int(o["indices"][c]) == i, where
        assert int(o["leaves"][c]) == leaf == int(s.cols[c][i]), where
        assert o["dirs"][c].tobytes() == dirs, where
        got = o["siblings"][c].tobytes()
        if got != sib:
            raise AssertionError(("siblings", where, "first differing level", [got[32 * l:32 * l + 32] == sib[32 * l:32 * l + 32] for l in range(nv)].index(False)))
        if boolean:
            a, b = int(s.cols[c][i & ~1]), int(s.cols[c][i | 1])
            want = (a + i * (b - a)) % P
        else:
            want = exact_ref.eval(s.cols[c].astype(np.uint64), pts[c])
        assert int(o["values"][c]) == want, ("value", where)


def _special(nv):
    N = 1 << nv
    idx = {0, 1, N - TAIL - 1, N - TAIL, N - TAIL + 1, N - 2, N - 1}
    for b in _boundaries(nv):
        idx |= {b - 1, b, b + 1}
    return sorted(idx)


def _index_sets(nv, ncols, seed):
    """per build one index per column: over the builds every column opens every special index, then random ones"""
    sp = _special(nv)
    sets = [[sp[(b + 5 * c) % len(sp)] for c in range(ncols)] for b in range(len(sp))]
    rng = np.random.default_rng(seed)
    return sets + [list(rng.integers(0, 1 << nv, ncols)) for _ in range(3)]


def _run_set(ctx, s, d, seed, index_sets=None, full_eval_first=True):
    """builds the set once per index set and checks everything; returns (gpu seconds, check seconds, last stats)"""
    gpu_s = chk_s = 0.0
    st = None
    for b, idx in enumerate(index_sets if index_sets is not None else _index_sets(s.nv, len(s.cols), seed)):
        boolean = not (full_eval_first and b == 0)
        pts = _points(s.nv, idx, seed + b, boolean)
        t0 = time.perf_counter()
        roots, o, st = _build(ctx, d, len(s.cols), s.nv, pts)
        t1 = time.perf_counter()
        _check_stats(s, st)
        _check(s, roots, o, pts, boolean)
        gpu_s += t1 - t0
        chk_s += time.perf_counter() - t1
    return gpu_s, chk_s, st


def _report(what, s, gpu_s, chk_s, builds):
    print(f"\n[merkle_exact] {what}: reference {s.ref_s:.1f} s ({s.hashes} hashes), {builds} builds + openings {gpu_s:.1f} s, "
          f"comparing (with one full eval per column) {chk_s:.1f} s")


@pytest.mark.parametrize("nv,period", MIXED)
def test_mixed_job_equals_the_reference(ctx, nv, period):
    """A group (kept up to 2^25, hinted but not taken at 2^26), six run-aware columns, a small-domain and a dense column in one
    job: every root, every opening and every opened value equal the reference; the counters show which path built what."""
    s = _set(nv, period)
    assert (len(s.G), len(s.H), len(s.R)) == ((5, 1, 6) if nv < 26 else (0, 3, 6))
    _hint(ctx, HINTS)
    d = _upload(ctx, s.cols)
    gpu_s, chk_s, st = _run_set(ctx, s, d, 100 * nv + period)
    ctx.dev_free(d)
    if nv < 26:
        assert st["cons_hashed"] < st["cons_dense_nodes"] // 50
    assert st["run_aware_hashed"] < st["run_aware_dense_nodes"] // 4
    _report(f"2^{nv}, loop of {period}", s, gpu_s, chk_s, len(_index_sets(nv, NCOLS, 0)))


@_FULL
def test_2p27_ignores_the_list_hints_and_keeps_the_tables(ctx):
    """Above RUN_MAX_LEAVES: a group-hinted loop, a column hinted three ways and a run-aware-hinted one are built densely and from
    the small-domain tables -- and still equal the reference."""
    nv = 27
    N = 1 << nv
    _evict(nv)
    step = np.arange(N, dtype=np.int64)
    changes = sorted(set(b + d for b in _boundaries(nv) + [1 << 26] for d in (-1, 0, 1)) | {N - 1})
    cols = [(0x1000 + 4 * (step % 12)).astype(np.uint32),
            np.repeat(np.arange(N // 512) % 128, 512).astype(np.uint32),
            (1 + np.searchsorted(np.array(changes), step, side="right")).astype(np.uint32)]
    del step
    hints = {"cons_group_mask": 0b011, "small_domain_mask": 0b010, "run_aware_mask": 0b110}
    s = _Set(cols, hints, nv).finish()
    assert (s.G, s.H, s.R) == ([], [1], [])
    _hint(ctx, hints)
    d = _upload(ctx, cols)
    sp = sorted(set(_special(nv)) | {(1 << 26) - 1, 1 << 26, (1 << 26) + 1})
    sets = [[sp[(b + 5 * c) % len(sp)] for c in range(3)] for b in range(len(sp))]
    gpu_s, chk_s, st = _run_set(ctx, s, d, 2700, index_sets=sets)
    ctx.dev_free(d)
    assert st["keccak_permutations"] == 3 * (2 * N - 1) - (N + N // 2)
    _report("2^27", s, gpu_s, chk_s, len(sets))


# ---------------------------------------------------------------- 2^22: what the context learnt from its earlier jobs
def _few_sets(nv, ncols, seed):
    sets = _index_sets(nv, ncols, seed)
    return sets[::6] + sets[-1:]


def test_2p22_after_a_job_of_another_size(ctx):
    """caps_for forgets the list sizes it learnt when the shape of the job changes: the long-loop set, a 2^16 job, the long-loop
    set again -- every build equals the reference, whatever room its lists started with."""
    nv = 22
    s = _set(nv, 8191)
    small = _Set(_group_columns(16, 12) + _other_columns(16), HINTS, 16).finish()
    _hint(ctx, HINTS)
    d, d16 = _upload(ctx, s.cols), _upload(ctx, small.cols)
    sets = _few_sets(nv, NCOLS, 1)
    g1 = _run_set(ctx, s, d, 2201, index_sets=sets)
    r1 = ctx.stats()["rebuilds"]
    rng = np.random.default_rng(16)
    _run_set(ctx, small, d16, 1601, index_sets=[list(rng.integers(0, 1 << 16, NCOLS)) for _ in range(2)])
    r2 = ctx.stats()["rebuilds"]
    g2 = _run_set(ctx, s, d, 2202, index_sets=sets)
    r3 = ctx.stats()["rebuilds"]
    ctx.dev_free(d)
    ctx.dev_free(d16)
    # A fresh shape starts with 256 entries per sub-list and level, and the probe's keys (every 16th wave: sub-lists 0 and 16 only)
    # are 8191 distinct tuples: the first build of the shape must run out of room and be repeated.  After the 2^16 job the
    # context has forgotten what it learnt, so the same builds are repeated exactly as often again.
    assert r1 >= 1 and r3 - r2 == r1, (r1, r2, r3)
    _report(f"2^22 after another size (rebuilds {r1}, {r2}, {r3})", s, g1[0] + g2[0], g1[1] + g2[1], 2 * len(sets))


def test_2p22_after_a_job_with_much_shorter_lists(ctx):
    """launch_level_hash sizes its grid from what the last build of the shape held (`expect`): the 12-step loop first (a few dozen
    entries per level), then the 8191-step loop on the same context and shape, then the short one again.  The long loop must
    really outgrow what the short one left (its first build is repeated: the lists and `expect` were the short loop's), and the
    short loop afterwards builds in the long loop's room without a repeat."""
    nv = 22
    a, b = _set(nv, 12), _set(nv, 8191)
    _hint(ctx, HINTS)
    da, db = _upload(ctx, a.cols), _upload(ctx, b.cols)
    sets = _few_sets(nv, NCOLS, 3)
    t, rebuilds = [], []
    for s, d, seed in ((a, da, 2211), (b, db, 2212), (a, da, 2213)):
        before = ctx.stats()["rebuilds"]
        t.append(_run_set(ctx, s, d, seed, index_sets=sets))
        rebuilds.append(ctx.stats()["rebuilds"] - before)
    # the 12-step loop leaves the group's lists at their 256 entries per sub-list; 8191 distinct tuples do not fit
    assert rebuilds[1] >= 1 and rebuilds[2] == 0, rebuilds
    ctx.dev_free(da)
    ctx.dev_free(db)
    _report(f"2^22 after shorter lists (rebuilds {rebuilds})", b, sum(x[0] for x in t), sum(x[1] for x in t), 3 * len(sets))


# ---------------------------------------------------------------- 2^21: keep / drop on both sides of both thresholds
def _probe_count(cols):
    """k_cons_leaf_insert with sample != 0: the distinct tuples among the leaves of every 16th chunk of 64 (CONS_SAMPLE)"""
    k = np.arange(cols[0].size)
    pick = (k // 64) % 16 == 0
    return M.GroupRef([c[pick] for c in cols]).distinct_tuples(0)


def _loop(N, period):
    return ((np.arange(N, dtype=np.int64) % period) * 1000003 % P).astype(np.uint32)  # (injective: period < p)


def _hidden(N, distinct):
    """0 in the chunks the probe looks at; elsewhere the first `distinct` leaves count 1, 2, 3 ... and the rest are 0"""
    k = np.arange(N)
    out = np.zeros(N, dtype=np.uint32)
    free = np.flatnonzero((k // 64) % 16 != 0)[:distinct]
    out[free] = 1 + np.arange(distinct)
    return out


DECIDE = {  # name: (the group's first column, probe count within, full count within, kept)
    "a_loop_2p19_at_both_thresholds": (lambda N: _loop(N, 1 << 19), lambda n, N: n == N // 64, lambda n, N: n == N // 4, True),
    "a_loop_33224_just_under_the_probes": (lambda N: _loop(N, 33224), lambda n, N: N // 64 - 64 <= n <= N // 64, lambda n, N: n == 33224, True),
    "b_loop_32785_just_over_the_probes": (lambda N: _loop(N, 32785), lambda n, N: N // 64 < n <= N // 64 + 64, lambda n, N: n == 32785, False),
    "c_hidden_from_the_probe_one_over_a_quarter": (lambda N: _hidden(N, N // 4), lambda n, N: n == 1, lambda n, N: n == N // 4 + 1, False),
    "c_hidden_from_the_probe_exactly_a_quarter": (lambda N: _hidden(N, N // 4 - 1), lambda n, N: n == 1, lambda n, N: n == N // 4, True),
}


@pytest.mark.parametrize("case", list(DECIDE))
def test_2p21_keep_or_drop_at_the_thresholds(ctx, case):
    """k_cons_decide: the probe (distinct tuples in every 16th chunk of 64 leaves) drops a group above npad / 64, the full pass
    above npad / 4.  Both counts are emulated here from those rules; kept or dropped, the roots are the reference's."""
    nv = 21
    N = 1 << nv
    first, probe_ok, full_ok, kept = DECIDE[case]
    _evict(nv)
    cols = [first(N), np.full(N, 7, dtype=np.uint32), np.repeat(rnd(1, N // 1000 + 1), 1000)[:N].astype(np.uint32)]
    hints = {"cons_group_mask": 0b011, "small_domain_mask": 0, "run_aware_mask": 0b100}
    probe = _probe_count(cols[:2])
    full = M.GroupRef(cols[:2]).distinct_tuples(0)
    assert probe_ok(probe, N) and full_ok(full, N), (probe, full)
    probe_drops = probe > N // 64
    assert kept == (not probe_drops and not full > N // 4)
    s = _Set(cols, hints, nv).finish()
    if not kept:  # what the counters of a dropped group must say: no content-addressed column, nothing hashed by that path
        s.G, s.group = [], None
    _hint(ctx, hints)
    ctx.set_option("cons_always", 1)  # (a context stops trying a group it dropped twice: not what is tested here)
    d = _upload(ctx, cols)
    sets = _index_sets(nv, 3, 9)[::5]
    rebuilds = []
    gpu_all = chk_all = 0.0
    for rep in range(3):
        before = ctx.stats()["rebuilds"]
        gpu_s, chk_s, st = _run_set(ctx, s, d, 2100 + rep, index_sets=sets[:1] if rep else sets, full_eval_first=rep == 0)
        rebuilds.append(ctx.stats()["rebuilds"] - before)
        gpu_all, chk_all = gpu_all + gpu_s, chk_all + chk_s
        assert st["cons_probe_distinct"] == (16 * probe if probe_drops else full)
        if not kept:
            assert st["cons_dense_nodes"] == 0
    ctx.dev_free(d)
    # the first build finds its lists too short (256 entries per sub-list to start with) or, dropped, its columns without a
    # slab, and is repeated; the context has learnt, and the later builds are not
    assert rebuilds[0] >= 1 and rebuilds[1:] == [0, 0], rebuilds
    _report(f"2^21 {case} (probe {probe}, full {full}, rebuilds {rebuilds})", s, gpu_all, chk_all, len(sets) + 2)


# ---------------------------------------------------------------- one real trace
TRACE_HINTS = {"small_domain_mask": (1 << 1) | (0x3f << 33) | (1 << 42), "run_aware_mask": (0x7fffffff << 2) | (3 << 40),
               "cons_group_mask": 1 | (1 << 1) | (0x7f << 33) | (1 << 42)}  # the prover's defaults (test_gpu_structure_schedule.HINTS)


@pytest.mark.parametrize("nv", [21])
def test_real_trace_every_column(ctx, nv):
    """programs.add_xor_loop through the device witness build with the prover's default hints: all 43 roots and one opening
    per column equal the reference computed from the host witness.  The register columns change every few steps -- millions
    of distinct nodes: this is the expensive reference (printed), and the only check of real register columns at a size where
    runs stage 2 rides in H(0).  Measured on the MI355X host: 6.55 M hashes and 4.8 s of reference at 2^21 (the test 5.8 s);
    2^22 passes too but costs 13.1 M hashes, 9.6 s of reference and 12.3 s in all -- more than the full-size config 4 test
    next to it (5.7 s) -- so it is left at 2^21."""
    from zigz_amd import host
    N = 1 << nv
    _evict(nv)
    tr = host.Trace(programs.add_xor_loop((N - 3) // 4), 0x1000, None, 2 * N)
    assert tr.num_vars == nv
    wit = tr.witness()
    s = _Set([wit[c].astype(np.uint32) for c in range(43)], TRACE_HINTS, nv).finish()
    assert (len(s.G), len(s.H), len(s.R)) == (10, 0, 33)
    _hint(ctx, TRACE_HINTS)
    d = ctx.dev_alloc(43 * N * 4)
    tr.witness_to_device(ctx, d, N)
    rng = np.random.default_rng(nv)
    sets = [list(rng.integers(0, N, 43)), [int(x) for x in rng.choice(_special(nv), 43)]]
    gpu_s, chk_s, st = _run_set(ctx, s, d, 4300 + nv, index_sets=sets)
    ctx.dev_free(d)
    _report(f"2^{nv} add_xor_loop, 43 columns", s, gpu_s, chk_s, len(sets))
