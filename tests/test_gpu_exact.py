"""The device sumcheck, eval, bind and half-sums entries against the exact host reference (tests/exact_ref.py) at every shape
the radix schedules take -- the production sizes 2^20 .. 2^28 included -- with worst-case values and edge challenges, and the
pinned-memory hand-offs of the radix sumcheck under concurrent contexts.

Radix sumcheck stages (api_mle.cpp radix_run): nv 11..18 one stage of k = nv - 8; 19..20 k = 10 and a 512 / 1024-entry tail;
21..28 a second stage of k = nv - 18 (<= 5: the fold's clamped path).  Radix eval (dev_eval_radix): nv 14..24, k1 = nv - 10."""
import threading

import numpy as np
import pytest

import exact_ref as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
GRID_NVS = (11, 13, 18, 19, 20, 21, 22, 23, 24)
# the other sizes: random values plus one worst-case pattern
WORST = {12: "alternating", 14: "last_pm1", 15: "block_pm1", 16: "ramp", 17: "all_pm1", 25: "block_pm1", 26: "last_pm1",
         27: "all_pm1"}


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    c = zigz_amd.Context(0)
    yield c
    c.close()


class Table:
    """a table uploaded to its own device allocation (16-byte aligned), at a 4-byte offset when off = 1"""

    def __init__(self, ctx, ev, off=0):
        self.ctx, self.n = ctx, len(ev)
        self.base = ctx.dev_alloc((self.n + 4) * 4)
        self.d = self.base + 4 * off
        ctx.upload(ev, self.d)

    def free(self):
        self.ctx.dev_free(self.base)


def same(got, want):
    r, pt, fe = got
    r0, pt0, fe0 = want
    return np.array_equal(r, r0) and np.array_equal(pt, pt0) and int(fe) == int(fe0) and \
        O.sumcheck_to_bytes(r, pt, fe) == O.sumcheck_to_bytes(r0, pt0, fe0)


def _sumcheck_cases(nv):
    if nv in GRID_NVS:
        return [(p, c) for p in E.PATTERNS for c in E.CHALLENGES]
    if nv == 28:
        return [("random", "fs")]
    return [("random", "fs"), ("random", "random"), (WORST[nv], "fs"), (WORST[nv], "pm1")]


# ---------------------------------------------------------------- single-table sumcheck, every nv 11..28
@pytest.mark.parametrize("nv", list(range(11, 29)))
def test_sumcheck_every_shape(ctx, nv):
    modes = (0, 1) if nv <= 24 else (0,)  # radix, and per_round_sumcheck = 1 up to 2^24
    bad = []
    by_pattern = {}
    for pat, ch in _sumcheck_cases(nv):
        by_pattern.setdefault(pat, []).append(ch)
    try:
        for pat, chs in by_pattern.items():
            ev = E.pattern(pat, nv)
            t = Table(ctx, ev)
            try:
                for ch in chs:
                    c = E.challenges(ch, nv)
                    want = E.sumcheck_prove(ev, c)
                    for mode in modes:
                        ctx.set_option("per_round_sumcheck", mode)
                        got = ctx.dev_sumcheck_prove(t.d, t.n, c)
                        if not same(got, want):
                            bad.append((pat, ch, mode))
            finally:
                t.free()
            del ev
    finally:
        ctx.set_option("per_round_sumcheck", 0)
    assert not bad, f"nv {nv}: (pattern, challenges, per_round) differ from the exact reference: {bad}"


# ---------------------------------------------------------------- eval, every nv 13..26 (fold / radix boundaries 13|14, 24|25)
def _points(nv):
    return {"zero": [0] * nv, "one": [1] * nv, "pm1": [P - 1] * nv, "lsb": [1] + [0] * (nv - 1),
            "random": list(O.splitmix64_field(0xE7 + nv, nv))}


@pytest.mark.parametrize("nv", list(range(13, 27)))
def test_eval_every_shape(ctx, nv):
    bad = []
    pts = _points(nv)
    tables = [("random", pts), (E.PATTERNS[1 + nv % 5], {k: pts[k] for k in ("pm1", "random")})]
    for pat, ps in tables:
        ev = E.pattern(pat, nv, seed=1)
        t = Table(ctx, ev)
        try:
            for name, pt in ps.items():
                want = E.eval(ev, pt)
                modes = (0, 1) if nv in (20, 24) else (0,)  # fold_eval = 1 too where the radix form would run
                for mode in modes:
                    ctx.set_option("fold_eval", mode)
                    got = ctx.dev_mle_eval(t.d, t.n, pt)
                    if got != want:
                        bad.append((pat, name, mode, got, want))
        finally:
            ctx.set_option("fold_eval", 0)
            t.free()
    assert not bad, f"nv {nv}: (pattern, point, fold_eval, got, want): {bad}"


def test_eval_unaligned_takes_the_fold_path(ctx):
    nv = 21
    ev = E.pattern("random", nv, seed=2)
    t = Table(ctx, ev, off=1)  # 4-byte aligned only: not the radix form
    try:
        for name, pt in _points(nv).items():
            assert ctx.dev_mle_eval(t.d, t.n, pt) == E.eval(ev, pt), name
    finally:
        t.free()


# ---------------------------------------------------------------- bind, bind + sums, half sums: nv 19..26
@pytest.mark.parametrize("nv", list(range(19, 27)))
def test_bind_and_half_sums(ctx, nv):
    n = 1 << nv
    ev = E.pattern(E.PATTERNS[nv % 6], nv, seed=3) if nv % 2 else E.pattern("random", nv, seed=3)
    t = Table(ctx, ev)
    out = ctx.dev_alloc((n // 2 + 4) * 4)
    try:
        s0, s1 = E.half_sums(ev)
        assert ctx.dev_mle_half_sums(t.d, n) == [s0 % P, s1 % P]
        for r in (0, 1, P - 1, int(O.splitmix64_field(0xB1 + nv, 1)[0])):
            want = E.bind(ev, r)
            ctx.dev_mle_bind(t.d, n, r, out)
            assert np.array_equal(ctx.download(out, n // 2), want), ("bind", r)
            h0, h1 = E.half_sums(want)
            assert ctx.dev_mle_bind_sums(t.d, n, r, out) == [h0 % P, h1 % P], ("bind_sums", r)
            assert np.array_equal(ctx.download(out, n // 2), want), ("bind_sums table", r)
    finally:
        ctx.dev_free(out)
        t.free()


# ---------------------------------------------------------------- one batch of every size 2^1 .. 2^24
def test_batch_every_size(ctx):
    nvs = list(range(1, 25))
    evs = [E.pattern(E.PATTERNS[i % len(E.PATTERNS)], nv, seed=4) for i, nv in enumerate(nvs)]
    tabs = [Table(ctx, ev) for ev in evs]
    fixed_sets = ("zero", "one", "pm1", "random")
    try:
        for fixed in (False, True):
            chs = [E.challenges(fixed_sets[i % 4], nv) for i, nv in enumerate(nvs)] if fixed else None
            got = ctx.dev_sumcheck_prove_batch([t.d for t in tabs], [t.n for t in tabs], chs)
            bad = [nv for i, nv in enumerate(nvs) if not same(got[i], E.sumcheck_prove(evs[i], chs[i] if fixed else None))]
            assert not bad, f"fixed challenges {fixed}: tables 2^nv differ from the exact reference: {bad}"
    finally:
        for t in tabs:
            t.free()


# ---------------------------------------------------------------- multi-column eval through a commit job
@pytest.mark.parametrize("ncols,nv,n_const", [(43, 21, 0), (43, 21, 24), (43, 21, 33), (4, 24, 3)])
def test_commit_job_eval_every_column(ctx, ncols, nv, n_const):
    """open_all's values are the evals of every column.  Constant columns under the run-aware hint are left out of the
    radix pass (EvalSkip); the fewer columns remain, the fewer row loops a thread takes (rloops 4 / 2 / 1)."""
    import zigz_amd
    N = 1 << nv
    cols = O.splitmix64_field(0xC0 + ncols + nv + n_const, ncols * N).reshape(ncols, N)
    hinted = list(range(ncols - n_const, ncols))
    for j, c in enumerate(hinted):
        cols[c, :] = (0, 1, P - 1, 12345)[j % 4]
    if ncols > 4:
        cols[1, :] = E.pattern("last_pm1", nv)
        cols[2, :] = E.pattern("block_pm1", nv)
    mask = 0
    for c in hinted:
        mask |= 1 << c
    pts = O.splitmix64_field(0xC1 + nv, ncols * nv).reshape(ncols, nv)
    pts[0, :] = P - 1
    ctx.set_option("run_aware_mask", mask)
    try:
        job = zigz_amd.CommitJob(ctx, cols=cols)
        job.roots()
        got = job.open_all(pts)
        job.end()
        assert ctx.stats()["eval_constant_columns"] == n_const
    finally:
        ctx.set_option("run_aware_mask", 0)
    bad = [c for c in range(ncols) if int(got["values"][c]) != E.eval(cols[c], pts[c])]
    assert not bad, f"columns whose opened value is not the eval: {bad}"


# ---------------------------------------------------------------- hand-offs under concurrent contexts
def test_concurrent_radix_hand_offs():
    """4 contexts, each 12 radix sumchecks at 2^18..2^20 (every first stage publishes 1024 sums over 4 workgroups), while a
    fifth builds 43-column commit jobs of 2^20; every proof must be the exact reference's.  A fixed count: a parity check."""
    import zigz_amd
    tables = {}
    for th in range(4):
        for i in range(12):
            nv = 18 + i % 3
            pat = ("random", "all_pm1", "block_pm1", "random")[i % 4]
            tables[th, i] = E.pattern(pat, nv, seed=100 * th + i)
    want = {key: E.sumcheck_prove(ev) for key, ev in tables.items()}
    got, errors = {}, []
    start = threading.Barrier(5)

    def prover(th):
        try:
            c = zigz_amd.Context(0)
            try:
                tabs = [Table(c, tables[th, i]) for i in range(12)]
                start.wait()
                for i, t in enumerate(tabs):
                    got[th, i] = c.dev_sumcheck_prove(t.d, t.n)
                for t in tabs:
                    t.free()
            finally:
                c.close()
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append((th, repr(e)))
            start.abort()

    def committer():
        try:
            c = zigz_amd.Context(0)
            try:
                cols = O.splitmix64_field(0xC077, 43 * (1 << 20)).reshape(43, 1 << 20)
                start.wait()
                roots = []
                for _ in range(3):
                    job = zigz_amd.CommitJob(c, cols=cols)
                    roots.append(job.roots().copy())
                    job.end()
                assert all(np.array_equal(r, roots[0]) for r in roots)
            finally:
                c.close()
        except Exception as e:  # noqa: BLE001
            errors.append(("commit", repr(e)))
            start.abort()

    threads = [threading.Thread(target=prover, args=(th,)) for th in range(4)] + [threading.Thread(target=committer)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    bad = sorted(key for key in tables if not same(got[key], want[key]))
    assert not bad, f"(thread, proof) differing from the exact reference: {bad}"
