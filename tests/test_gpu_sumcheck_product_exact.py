"""The batched product sumcheck prover (sumcheck_product.hip, api_product.cpp, product_host.hpp) at the sizes where its code takes
a path that test_gpu_sumcheck_product.py never reaches -- every output word (claimed sum, all (d + 1) v round words, point, factor
evals, final eval) of every proof against the numpy reference (sumcheck_product_ref.prove), R.same, no tolerance, nothing sampled:

  2^21, 2^22, 2^23   k_product_finish adds cnt = m / 8192 partials with a loop strided by 256 threads: cnt = 256 at 2^21 (every
                     thread exactly one), 512 at 2^22 (the first second trip; the later rounds walk cnt down through 256 .. 1 in
                     the same proof), 1024 at 2^23 (four trips).  Each large proof is also checked the way a verifier sees it
                     (claim chain, factor evals == exact_ref.eval at the reversed point, their product): the one check that
                     shares no restatement of the prover with the code under test.
  big behind small   a 512-workgroup instance whose partials start at an odd first_wg, the same batch reversed, a small batch
                     and the first again: nothing is zeroed in between
  fresh context      the workspaces (WS_PRODUCT, WS_PRODUCT_WORK, WS_PRODUCT_IN) grow between calls of one context
  4096 instances     ZIGZ_BATCH_MAX live instances of one partial workgroup each (find_first_wg over 4096 descriptors, a finish
                     grid of 4096 workgroups, the pinned region beyond the context's fixed one), and sizes 2^10 .. 2^13 mixed:
                     a quarter is never live, the live set shrinks in stages, a descriptor's position is not its result slot
  field edges        tables and challenges of 0, 1 and p - 1 at 2^11, 2^13, 2^14 (see test_field_edges)

The three 2^23 tables are generated and uploaded once per module; the 2^21 and 2^22 instances are prefixes of them.  A reference
proof is computed once (Refs) and shared by the tests that compare against it.

Seconds per test on the GPU host (pytest --durations=0; the reference's proof and the verifier's check included; the whole
module 2.9 s, next to test_gpu_sumcheck_product.py's 0.3 s):
  setup of the first test (three 2^23 tables generated and uploaded)            0.50
  test_large_single  2^21: d = 1  0.07, d = 2  0.12, d = 3  0.17, d = 3 fixed  0.17
                     2^22: d = 1  0.11, d = 2  0.21, d = 3  0.34, d = 2 fixed  0.21        2^23: d = 3  0.76
  test_big_instances_behind_small_ones  0.03 (every reference shared with the singles)
  test_workspaces_grow_on_a_fresh_context  0.05      test_4096_instances  0.05, 0.05
  test_field_edges  2^11  0.04, 2^13  0.06, 2^14  0.09
The large singles are reference time: R.prove and the three exact_ref.eval folds run on the host over the same 2^21 .. 2^23
values; the prover's own calls are milliseconds."""
import pytest

import oracle_lib as O
import sumcheck_product_ref as R
from test_gpu_sumcheck_product import DevTables

pytestmark = pytest.mark.gpu

P = O.P_BB
BATCH_MAX = 4096  # ZIGZ_BATCH_MAX
BIG = 23
# (log2 n, d, fixed challenges?): 2^21 and 2^22 at every degree with Fiat-Shamir and one degree each with fixed challenges
LARGE = [(21, 1, False), (21, 2, False), (21, 3, False), (21, 3, True),
         (22, 1, False), (22, 2, False), (22, 3, False), (22, 2, True), (23, 3, False)]


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    c = zigz_amd.Context(0)
    yield c
    c.close()


class Refs:
    """the module's three random 2^23 tables, and the reference's proof of the first d of them cut to 2^nv, each computed once"""

    def __init__(self):
        self.tables = [O.splitmix64_field(61000 + 17 * j, 1 << BIG) for j in range(3)]
        self.proofs = {}

    def factors(self, nv, d):
        return [t[:1 << nv] for t in self.tables[:d]]

    def challenges(self, nv):
        return O.splitmix64_field(62000 + nv, nv)

    def proof(self, nv, d, fixed=False):
        key = (nv, d, fixed)
        if key not in self.proofs:
            self.proofs[key] = R.prove(self.factors(nv, d), self.challenges(nv) if fixed else None)
        return self.proofs[key]


@pytest.fixture(scope="module")
def refs():
    return Refs()


@pytest.fixture(scope="module")
def dev(ctx, refs):
    d = DevTables(ctx, refs.tables)
    yield d
    d.free()


@pytest.mark.parametrize("nv,d,fixed", LARGE)
def test_large_single(ctx, refs, dev, nv, d, fixed):
    n = 1 << nv
    ch = [refs.challenges(nv)] if fixed else None
    got, = ctx.dev_sumcheck_prove_product_batch([dev.ptrs[:d]], [n], ch)
    assert R.same(got, refs.proof(nv, d, fixed)), (nv, d, fixed)
    # the verifier's view, independent of the reference prover
    R.check_proof(refs.factors(nv, d), got, fiat_shamir=not fixed, mle_eval=R.exact_mle_eval)
    if d == 1:  # bytes-equal to the linear batched prover
        (rounds, point, fe), = ctx.dev_sumcheck_prove_batch(dev.ptrs[:1], [n], ch)
        assert rounds.tobytes() == got[1].tobytes() and point.tobytes() == got[2].tobytes() and fe == got[4] == int(got[3][0])
    assert dev.unchanged()


def test_big_instances_behind_small_ones(ctx, refs, dev):
    """first_wg of the 2^22 instances is 1 and 770, of the 2^21 one 514: their 512 / 256 partial sets start at odd offsets, and
    in the reversed batch at others; the last instance reads the d = 3 instance's first factor"""
    shape = [(13, 2), (22, 3), (11, 1), (21, 2), (5, 3), (22, 1)]
    ptrs = [dev.ptrs[:d] for _, d in shape]
    ns = [1 << nv for nv, _ in shape]
    want = [refs.proof(nv, d) for nv, d in shape]
    batch = ctx.dev_sumcheck_prove_product_batch(ptrs, ns)
    for i in range(len(shape)):
        assert R.same(batch[i], want[i]), i
        alone, = ctx.dev_sumcheck_prove_product_batch([ptrs[i]], [ns[i]])
        assert R.same(alone, want[i]), i
    other = ctx.dev_sumcheck_prove_product_batch(ptrs[::-1], ns[::-1])
    small = ctx.dev_sumcheck_prove_product_batch([ptrs[2], ptrs[0]], [ns[2], ns[0]])
    again = ctx.dev_sumcheck_prove_product_batch(ptrs, ns)
    for i in range(len(shape)):
        assert R.same(other[len(shape) - 1 - i], want[i]) and R.same(again[i], want[i]), i
    assert R.same(small[0], want[2]) and R.same(small[1], want[0])
    assert dev.unchanged()


def test_workspaces_grow_on_a_fresh_context(refs):
    """2^11, then 2^22 at d = 3, then 2^11 again on a context that has run nothing: every workspace of the prover grows under it;
    the same through the host form with 2^14"""
    import zigz_amd
    small, big, mid = refs.factors(11, 2), refs.factors(22, 3), refs.factors(14, 3)
    with zigz_amd.Context(0) as c:
        d = DevTables(c, big)
        try:
            for ptrs, n, want in ((d.ptrs[:2], 1 << 11, refs.proof(11, 2)), (d.ptrs, 1 << 22, refs.proof(22, 3)),
                                  (d.ptrs[:2], 1 << 11, refs.proof(11, 2))):
                got, = c.dev_sumcheck_prove_product_batch([ptrs], [n])
                assert R.same(got, want), n
            for fs, want in ((small, refs.proof(11, 2)), (mid, refs.proof(14, 3)), (small, refs.proof(11, 2))):
                got, = c.sumcheck_prove_product_batch([fs])
                assert R.same(got, want), len(fs[0])
            assert d.unchanged()
        finally:
            d.free()
    assert c.h is None  # closed


@pytest.fixture(scope="module")
def types(ctx):
    """8 instance types, degrees cycling 1, 2, 3: 15 distinct 2^13 tables on the device (480 KiB), cut to the size a call asks for"""
    degs = [1 + t % 3 for t in range(8)]
    tabs = [[O.splitmix64_field(63000 + 100 * t + j, 1 << 13) for j in range(d)] for t, d in enumerate(degs)]
    d = DevTables(ctx, [f for fs in tabs for f in fs])
    ptrs, o = [], 0
    for k in degs:
        ptrs.append(d.ptrs[o: o + k])
        o += k
    yield tabs, ptrs, d
    d.free()


@pytest.mark.parametrize("logs", [[11], [10, 11, 12, 13]], ids=["all_2p11", "2p10_to_2p13"])
def test_4096_instances(ctx, types, logs):
    """instance i is of type i % 8 and 2^logs[i % len(logs)] long (so a type has one size per call): 8 reference proofs, and
    every one of the 4096 proofs compared with its type's"""
    tabs, ptrs, d = types
    nv = [logs[t % len(logs)] for t in range(8)]
    want = [R.prove([f[:1 << nv[t]] for f in tabs[t]]) for t in range(8)]
    got = ctx.dev_sumcheck_prove_product_batch([ptrs[i % 8] for i in range(BATCH_MAX)], [1 << nv[i % 8] for i in range(BATCH_MAX)])
    assert len(got) == BATCH_MAX
    wrong = [i for i in range(BATCH_MAX) if not R.same(got[i], want[i % 8])]
    assert not wrong, (len(wrong), wrong[:16])
    assert d.unchanged()


@pytest.mark.parametrize("nv", [11, 13, 14])
def test_field_edges(ctx, nv):
    """One partial workgroup, one full chunk, two chunks.  R.PATTERN_SETS x d = 1..3 x R.EDGE_CHALLENGES: 126 instances over 8
    tables, and the constructed R.REDUCE_EDGE over two more.  The entry fixes the challenges of a whole call or of none, so a
    size is two calls: the 22 Fiat-Shamir instances and the 105 with fixed challenges.  What the cases are for
    (tests/test_sumcheck_product_cpu.py counts that they reach it):
      step_down with challenges of 1   every first bind is add_mod(p - 1, 1): 0, not p
      constant tables (all_pm1)        every sub_mod(b, a) has b == a, and every monty_reduce a zero product (hi == u == 0)
      last_pm1                         the only non-zero term is the last component of the last vector of the last workgroup
      challenges 0 / 1                 the bound table is a plain copy of the low / high half: a pass that read the wrong
                                       quarter (q + m/4 for q + m/2) shows as a whole-table difference in the next round's sums
      p - 1, and 0 / p - 1 in turn     the bound table is 2a - b: host_to_mont(p - 1) and the largest products
      R.REDUCE_EDGE (1, p - 1, .. times 1)  a lane's deferred low-word sum is 2p (2^11; a multiple of p at every size): the only
                                       monty_reduce whose high word equals the subtracted word with a non-zero argument"""
    names = R.edge_pattern_names()
    tabs = {n: R.pattern(n, nv) for n in names}
    d = DevTables(ctx, [tabs[n] for n in names])
    try:
        ptr = dict(zip(names, d.ptrs))
        cases = R.edge_cases(nv) + [(R.REDUCE_EDGE, "fs")]
        assert len(cases) == 127
        for fs_call in (True, False):
            call = [(ps, c) for ps, c in cases if (c == "fs") == fs_call]
            ch = None if fs_call else [R.edge_challenges(c, nv) for _, c in call]
            got = ctx.dev_sumcheck_prove_product_batch([[ptr[n] for n in ps] for ps, _ in call], [1 << nv] * len(call), ch)
            assert len(got) == len(call) == (22 if fs_call else 105)
            for g, (ps, c) in zip(got, call):
                assert R.same(g, R.prove([tabs[n] for n in ps], R.edge_challenges(c, nv))), (ps, c)
        assert d.unchanged()
    finally:
        d.free()
