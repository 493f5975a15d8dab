"""Batched sumcheck and Lasso provers on the GPU (zigz_dev_sumcheck_prove_batch, zigz_sumcheck_prove_batch,
zigz_lasso_prove_batch): every table of a batch gives the bytes of its own single call, the error of the first failing
table comes with that table's index, and nothing else on the context is disturbed."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_MAX = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


def _bytes(r, p, fe):
    return O.sumcheck_to_bytes(r, p, fe)


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


def _mixed(k, seed, max_log):
    rng = np.random.default_rng(seed)
    logs = [int(x) for x in rng.integers(1, max_log + 1, size=k)]
    logs[0] = max_log
    if k > 2:
        logs[1] = 1
    ns = [1 << v for v in logs]
    return ns, [O.splitmix64_field(seed * 1000 + i, n) for i, n in enumerate(ns)]


def _check_against_single(ctx, tables, out, chs=None, singles=None):
    for i, t in enumerate(tables):
        n = len(t)
        if n <= ORACLE_MAX:
            exp = O.sumcheck_prove(P, t, chs[i] if chs is not None else None)
            assert _bytes(*out[i]) == _bytes(*exp), (i, n)
        else:
            assert _bytes(*out[i]) == _bytes(*singles[i]), (i, n)
            _claim_chain(t, *out[i])


def _claim_chain(t, rounds, point, fe):
    """the verifier's claim chain (orc_sumcheck_verify) with the final check at reverse(point), where the reference's
    final_eval lives; the oracle's own verdict is then exactly whether eval(point) happens to agree"""
    claim = O.mle_sum(P, t)
    for j in range(len(point)):
        c0, c1 = int(rounds[2 * j]), int(rounds[2 * j + 1])
        assert (2 * c0 + c1) % P == claim, j
        claim = (c0 + c1 * int(point[j])) % P
    assert claim == fe == O.mle_eval(P, t, [int(x) for x in point][::-1])
    assert O.sumcheck_verify(P, t, O.mle_sum(P, t), rounds, point, fe) == (O.mle_eval(P, t, [int(x) for x in point]) == fe)


@pytest.mark.parametrize("k,seed", [(1, 11), (3, 12), (16, 13)])
def test_dev_and_host_batch_match_single_calls(ctx, k, seed):
    ns, tables = _mixed(k, seed, 22)
    d = DevTables(ctx, tables)
    try:
        singles = [ctx.dev_sumcheck_prove(p, n) if n > ORACLE_MAX else None for p, n in zip(d.ptrs, ns)]
        out = ctx.dev_sumcheck_prove_batch(d.ptrs, ns)
        _check_against_single(ctx, tables, out, singles=singles)
        chs = [O.splitmix64_field(seed * 31 + i, n.bit_length() - 1) for i, n in enumerate(ns)]
        out_f = ctx.dev_sumcheck_prove_batch(d.ptrs, ns, challenges=chs)
        for i, t in enumerate(tables):
            if len(t) <= ORACLE_MAX:
                assert _bytes(*out_f[i]) == _bytes(*ctx.sumcheck_prove(t, chs[i])) == _bytes(*O.sumcheck_prove(P, t, chs[i]))
            else:
                assert _bytes(*out_f[i]) == _bytes(*ctx.dev_sumcheck_prove(d.ptrs[i], len(t), challenges=chs[i]))
    finally:
        d.free()
    small = [t for t in tables if len(t) <= ORACLE_MAX] or [O.splitmix64_field(5, 8)]
    out_h = ctx.sumcheck_prove_batch(small)
    _check_against_single(ctx, small, out_h)


def test_degenerate_shapes(ctx):
    # 4096 tables of 2 elements (the limit), the same pointer twice, a table 16 bytes into a larger buffer
    tables = [O.splitmix64_field(70000 + i, 2) for i in range(4096)]
    d = DevTables(ctx, tables)
    try:
        out = ctx.dev_sumcheck_prove_batch(d.ptrs, [2] * 4096)
        for i in range(0, 4096, 97):
            assert _bytes(*out[i]) == _bytes(*O.sumcheck_prove(P, tables[i]))
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_sumcheck_prove_batch(d.ptrs + d.ptrs[:1], [2] * 4097)
        assert e.value.code == E.INVALID_ARGUMENT
        assert ctx.dev_sumcheck_prove_batch([], []) == []
    finally:
        d.free()
    t = O.splitmix64_field(77, 1 << 13)
    d = DevTables(ctx, [t], extra_offset=4)  # 16 bytes into the buffer
    try:
        out = ctx.dev_sumcheck_prove_batch([d.ptrs[0], d.ptrs[0]], [1 << 13, 1 << 13])
        exp = _bytes(*O.sumcheck_prove(P, t))
        assert _bytes(*out[0]) == exp and _bytes(*out[1]) == exp
        with pytest.raises(E.ZigzError) as e:  # 4 bytes off: not 16-byte aligned
            ctx.dev_sumcheck_prove_batch([d.ptrs[0], d.ptrs[0] + 4], [1 << 13, 1 << 12])
        assert e.value.code == E.INVALID_ARGUMENT and e.value.bad_index == 1
    finally:
        d.free()


def test_batch_errors_name_the_first_failing_table(ctx):
    tables = [O.splitmix64_field(900 + i, 16) for i in range(4)]
    d = DevTables(ctx, tables)
    try:
        for ns, code, idx in [([16, 16, 12, 16], E.LENGTH_NOT_POWER_OF_TWO, 2), ([16, 16, 16, 1], E.NO_VARIABLES, 3),
                              ([16, 1, 12, 16], E.NO_VARIABLES, 1)]:
            with pytest.raises(E.ZigzError) as e:
                ctx.dev_sumcheck_prove_batch(d.ptrs, ns)
            assert e.value.code == code and e.value.bad_index == idx
        chs = [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, P, 4], [1, 2, 3, P + 5]]
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_sumcheck_prove_batch(d.ptrs, [16] * 4, challenges=chs)
        assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 2
    finally:
        d.free()
    bad = [t.copy() for t in tables]
    bad[1][5] = P
    with pytest.raises(E.ZigzError) as e:
        ctx.sumcheck_prove_batch(bad)
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    with pytest.raises(E.ZigzError) as e:  # table 2's length fails first in its own call, but table 1 is read before it
        ctx.sumcheck_prove_batch([tables[0], bad[1], tables[2][:12]])
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    with pytest.raises(E.ZigzError) as e:
        ctx.sumcheck_prove_batch([tables[0], tables[1], tables[2][:12]])
    assert e.value.code == E.LENGTH_NOT_POWER_OF_TWO and e.value.bad_index == 2


def test_batch_single_commit_batch_on_one_context(ctx):
    import zigz_amd
    ns, tables = _mixed(5, 21, 16)
    exp = [_bytes(*O.sumcheck_prove(P, t)) for t in tables]
    d = DevTables(ctx, tables)
    try:
        first = ctx.dev_sumcheck_prove_batch(d.ptrs, ns)
        one = ctx.dev_sumcheck_prove(d.ptrs[0], ns[0])
        nv = 11
        cols = np.stack([O.splitmix64_field(4000 + c, 1 << nv) for c in range(43)])
        cexp = O.generate_commitments(P, O.Transcript(), cols, fast=True)
        job = zigz_amd.CommitJob(ctx, cols=cols)
        roots = job.roots()
        job.end()
        second = ctx.dev_sumcheck_prove_batch(d.ptrs, ns)
    finally:
        d.free()
    assert np.array_equal(roots, cexp["roots"])
    assert _bytes(*one) == exp[0]
    assert [_bytes(*x) for x in first] == exp and [_bytes(*x) for x in second] == exp


def test_single_batch_and_degree_one_product_give_one_proof(ctx):
    """the three provers share one host round step and one tail: tail only (2), the 1024 hand-over boundary, the first live size
    (2048) and one size with a bind round before the hand-over (4096) give byte-identical proofs from each of them"""
    ns = [2, 1024, 2048, 4096]
    tables = [O.splitmix64_field(88000 + i, n) for i, n in enumerate(ns)]
    d = DevTables(ctx, tables)
    try:
        single = [ctx.dev_sumcheck_prove(p, n) for p, n in zip(d.ptrs, ns)]
        batch = ctx.dev_sumcheck_prove_batch(d.ptrs, ns)
        product = ctx.dev_sumcheck_prove_product_batch([[p] for p in d.ptrs], ns)
    finally:
        d.free()
    for i, t in enumerate(tables):
        claimed, rounds, point, evals, fe = product[i]
        exp = _bytes(*single[i])
        assert exp == _bytes(*O.sumcheck_prove(P, t)), ns[i]
        assert _bytes(*batch[i]) == exp, ns[i]
        assert _bytes(rounds, point, fe) == exp and int(evals[0]) == fe, ns[i]
        assert claimed == (int(rounds[0]) + (int(rounds[0]) + int(rounds[1])) % P) % P == O.mle_sum(P, t), ns[i]


def _lasso_case(seed, bits, nq, w, mapping):
    rng = np.random.default_rng(seed)
    n_in, n_out = w
    if (n_in, n_out) == (2, 1):
        tab = np.asarray(O.build_table(P, seed % 3, bits), dtype=np.uint64)
    else:
        tab = rng.integers(0, P, size=(1 << (2 * bits), n_in + n_out), dtype=np.uint64)
    idx = rng.integers(0, len(tab), size=nq)
    q = tab[idx]
    return dict(table=tab, queries=q, n_in=n_in, n_out=n_out, mapping=[int(x) for x in idx] if mapping else None)


def _lasso_same(got, exp):
    assert got["nv"] == exp["nv"]
    assert np.array_equal(got["rounds"], exp["rounds"]) and np.array_equal(got["point"], exp["point"])
    assert got["final_eval"] == exp["final_eval"]
    assert got["query_commit"] == exp["query_commit"] and got["table_commit"] == exp["table_commit"]


def test_lasso_batch_matches_oracle(ctx):
    cases = []
    for i, (w, nq, mp) in enumerate([((2, 1), 1000, False), ((1, 1), 37, True), ((3, 2), 4096, False), ((2, 1), 3, True),
                                     ((2, 1), 5000, True), ((3, 2), 2, False), ((1, 1), 2049, False)]):
        cases.append(_lasso_case(300 + i, 4 if w == (2, 1) else 3, nq, w, mp))
    got = ctx.lasso_prove_batch(cases)
    for c, g in zip(cases, got):
        exp = O.lasso_prove(P, c["table"], c["queries"], c["n_in"], c["n_out"], mapping=c["mapping"])
        _lasso_same(g, exp)


def test_lasso_batch_golden_vectors_in_one_batch(ctx):
    G = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    es = [e for e in G["lasso"] if e["p"] == str(P)]
    assert es
    cases = [dict(table=O.build_table(P, e["kind"], e["bits"]), queries=np.array([[int(x) for x in r] for r in e["queries"]], dtype=np.uint64))
             for e in es]
    got = ctx.lasso_prove_batch(cases)
    for e, g in zip(es, got):
        assert g["nv"] == e["nv"] and g["final_eval"] == int(e["final_eval"])
        assert [int(x) for x in g["rounds"]] == [int(x) for x in e["rounds"]]
        assert [int(x) for x in g["point"]] == [int(x) for x in e["point"]]
        assert g["query_commit"].hex() == e["query_commit"] and g["table_commit"].hex() == e["table_commit"]


def test_lasso_batch_errors(ctx):
    ok = _lasso_case(1, 3, 20, (2, 1), False)
    tab, q = ok["table"], ok["queries"]
    for bad, code in [(dict(table=tab, queries=np.zeros((0, 3), dtype=np.uint64)), E.NO_QUERIES),
                      (dict(table=tab, queries=q[:1]), E.NO_VARIABLES),
                      (dict(table=tab[:3], queries=q[:2]), E.LENGTH_NOT_POWER_OF_TWO),
                      (dict(table=tab, queries=q[:2], mapping=[0]), E.MAPPING_LENGTH_MISMATCH),
                      (dict(table=tab, queries=q[:2], mapping=[1 << 20, 0]), E.INVALID_MAPPING),
                      (dict(table=tab, queries=tab[[1, 2]], mapping=[1, 1]), E.QUERY_TABLE_MISMATCH)]:
        for where in (0, 2):
            batch = [ok, ok, ok]
            batch[where] = bad
            with pytest.raises(E.ZigzError) as e:
                ctx.lasso_prove_batch(batch)
            assert e.value.code == code and e.value.bad_index == where, (code, where)
    nc = dict(table=tab.copy(), queries=q)
    nc["table"][3, 1] = P
    with pytest.raises(E.ZigzError) as e:
        ctx.lasso_prove_batch([ok, nc, dict(table=tab, queries=q[:1])])
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    # after the errors the context still proves
    _lasso_same(ctx.lasso_prove_batch([ok])[0], O.lasso_prove(P, tab, q))
