"""The product trees and the grand-product argument at 2^16 to 2^23 words and at 4096 instances, word for word against numpy and
grand_product_ref.py: the sizes at which the tree schedule takes a second pass of fewer than three levels, three full passes and a
fourth pass, the host form's download makes a second and a third trip, the layers' zero-checks read a `hi` weight stage no shorter
than `lo` (layers 20 and 21 of a 2^22 column), several tall columns of different heights share the per-layer runs, and a
grand-product call stands between the other families' calls on one context.  Every comparison is exact.

No random column of this file holds a zero word (col() asserts it, the fixtures assert the references' products): a zero makes
every layer above it zero and hides errors there."""
import functools

import numpy as np
import pytest

import grand_product_ref as G
import oracle_lib as O
import test_gpu_sumcheck_family_one_context as F
from test_gpu_grand_product import DEFERRED, GUARD, GUARD_WORDS, Dev, dev_layers, product, prove_dev, verify_dev

pytestmark = pytest.mark.gpu

P = O.P_BB
TOP_LOG2 = 11  # gp::TOP_LOG2: k_gp_top takes a tree from its first layer of at most 2^11 words
MAX_FUSED = 3  # gp::MAX_FUSED
BATCH_MAX = 4096  # ZIGZ_BATCH_MAX


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    with zigz_amd.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def col(v, seed=0):
    """a random column of 2^v words without a zero word, computed once and read-only"""
    c = O.splitmix64_field(26000 + 41 * v + 1009 * seed, 1 << v)
    assert c.all(), "a zero word in a random column: pick another seed"
    c.flags.writeable = False
    return c


@pytest.fixture(scope="module", autouse=True)
def release_columns():
    """the columns (about 200 MB of host memory) go with the module, not with the session"""
    yield
    col.cache_clear()


def frozen(a):
    a.flags.writeable = False
    return a


def passes(v):
    """the fused levels of the passes that a column of 2^v words takes, as trees_queue schedules them"""
    out, J = [], v
    while J > TOP_LOG2:
        out.append(min(MAX_FUSED, J - TOP_LOG2))
        J -= out[-1]
    return out


def whole(ctx, d, tables):
    """every word of a Dev in one download, and the word at which each table starts"""
    at = [(p - d.base) // 4 for p in d.ptrs]
    return ctx.download(d.base, at[-1] + len(tables[-1])), at


def irregular_order(k, kinds, seed):
    """k indices below `kinds` in an irregular order: every index used, no two neighbours equal"""
    which = [int(x) for x in np.random.default_rng(seed).integers(0, kinds, k)]
    for i in range(1, k):
        if which[i] == which[i - 1]:
            which[i] = (which[i] + 1) % kinds
    assert set(which) == set(range(kinds)) and all(a != b for a, b in zip(which, which[1:]))
    return which


# ---------------------------------------------------------------- 1: the trees, device form
# 16: passes of 3 and 2 levels; 18: 3, 3, 1; 19: 3, 3, 2; 20: three full passes, 128 workgroups; 21 and 22: a fourth pass (1 and 2
# levels), 256 and 512 workgroups in the first
TREE_SIZES = [16, 18, 19, 20, 21, 22]
MIXED_TREES = [20, 12, 18, 3, 13, 21, 16]
assert [passes(v) for v in TREE_SIZES] == [[3, 2], [3, 3, 1], [3, 3, 2], [3, 3, 3], [3, 3, 3, 1], [3, 3, 3, 2]]


@pytest.fixture(scope="module")
def trees():
    """v -> (column, its tree buffer with GUARD in word n - 1)"""
    out = {}
    for v in sorted(set(TREE_SIZES + MIXED_TREES)):
        t = frozen(G.tree_buffer(col(v), fill=GUARD))
        assert int(t[len(t) - 2]) != 0
        out[v] = (col(v), t)
    return out


@pytest.mark.parametrize("v", TREE_SIZES)
def test_layers_of_a_tall_column_equal_numpy(ctx, trees, v):
    c, want = trees[v]
    got, = dev_layers(ctx, [c])  # (checks word n - 1, the guard words behind the buffer and the column)
    assert np.array_equal(got, want)
    assert int(got[len(got) - 2]) == product(c)


def test_layers_of_a_mixed_tall_batch_and_its_reverse(ctx, trees):
    """A tall column first, so the descriptors behind it have a large first_wg (128 and more); the columns of 2^12 and 2^13 are in
    the first pass only, 2^16 in two, 2^18 in three, while 2^20 and 2^21 go on: every pass has another set of descriptors"""
    assert [len(passes(v)) for v in MIXED_TREES] == [3, 1, 3, 0, 1, 4, 2]
    for order in (MIXED_TREES, MIXED_TREES[::-1]):
        got = dev_layers(ctx, [trees[v][0] for v in order])
        for g, v in zip(got, order):
            assert np.array_equal(g, trees[v][1]), v


def many_columns(sizes, per_size, seed):
    """(which, columns): BATCH_MAX indices in an irregular order into per_size distinct columns of every size"""
    cols = [col(v, 1 + s) for s in range(per_size) for v in sizes]  # column c has 2^sizes[c % len(sizes)] words
    which = irregular_order(BATCH_MAX, len(cols), seed)
    lengths = [len(cols[w]) for w in which]
    assert lengths != sorted(lengths) and lengths != sorted(lengths, reverse=True)
    return which, cols


@pytest.fixture(scope="module")
def many_trees():
    which, cols = many_columns([11, 12, 13, 14], 6, 5)
    want = [frozen(np.concatenate([G.tree_buffer(c, fill=GUARD), np.full(GUARD_WORDS, GUARD, dtype=np.uint64)])) for c in cols]
    assert all(int(t[len(c) - 2]) != 0 for t, c in zip(want, cols))
    return which, cols, want


def test_layers_of_4096_columns(ctx, many_trees):
    """ZIGZ_BATCH_MAX columns of 2^11 to 2^14 words in one call: find_first_wg searches 3047 descriptors (the columns above 2^11) in
    the k_gp_layers launch, k_gp_top runs 4096 workgroups.  The buffers lie one behind the other with 8 guard words each, so the whole region is compared
    at once: the trees, every word n - 1 and every guard word"""
    which, cols, want = many_trees
    ins = [cols[w] for w in which]
    assert sum(len(c) > 1 << TOP_LOG2 for c in ins) == 3047
    blank ={len(c): np.full(len(c) + GUARD_WORDS, GUARD, dtype=np.uint64) for c in cols}
    d = Dev(ctx, ins)
    outs = Dev(ctx, [blank[len(c)] for c in ins])
    try:
        ctx.dev_product_layers_batch(d.ptrs, [len(c) for c in ins], outs.ptrs)
        got, at = whole(ctx, outs, [want[w] for w in which])
        assert at[1] == len(want[which[0]]), "the buffers are contiguous"
        if not np.array_equal(got, np.concatenate([want[w] for w in which])):
            bad = [i for i, (a, w) in enumerate(zip(at, which)) if not np.array_equal(got[a: a + len(want[w])], want[w])]
            raise AssertionError("trees (or their guard words) differ: %d of them, the first at %d (2^%d)"
                                 % (len(bad), bad[0], len(ins[bad[0]]).bit_length() - 1))
        back, at = whole(ctx, d, ins)
        assert all(np.array_equal(back[a: a + len(c)], c) for a, c in zip(at, ins)), "a column was written"
    finally:
        d.free()
        outs.free()


# ---------------------------------------------------------------- 2: the trees, host form, across download chunks
DOWNLOAD_WORDS = (32 << 20) // 4  # api_grand_product.cpp: DOWNLOAD_BYTES / 4, the words of one trip of trees_host


def packed_offsets(ns):
    """batch_host.hpp: every column starts at a multiple of 4 words"""
    at = [0]
    for n in ns:
        at.append(at[-1] + (n + 3) // 4 * 4)
    return at


@pytest.fixture(scope="module")
def host_trees():
    """name -> (column, its tree buffer with 0 in word n - 1)"""
    named = {"22a": col(22), "22b": col(22, 1), "23": col(23), "2": col(2), "11": col(11)}
    out = {}
    for name, c in named.items():
        t = frozen(G.tree_buffer(c, fill=0))
        assert int(t[len(t) - 2]) != 0
        out[name] = (c, t)
    return out


def check_host_trees(ctx, host_trees, names):
    got = ctx.product_layers_batch([host_trees[x][0] for x in names])
    assert len(got) == len(names)
    for g, x in zip(got, names):
        assert np.array_equal(g, host_trees[x][1]), x


def test_host_trees_straddle_two_chunk_boundaries(ctx, host_trees):
    names = ["22a", "23", "2", "22b"]
    ns = [len(host_trees[x][0]) for x in names]
    at = packed_offsets(ns)
    assert ns == [1 << 22, 1 << 23, 4, 1 << 22] and at[:4] == [0, 1 << 22, 3 << 22, (3 << 22) + 4]
    # three trips; the first boundary falls inside column 1, the second leaves column 3's last four words -- its product among them,
    # at word n - 2 -- alone in the third
    assert 2 * DOWNLOAD_WORDS < at[4] <= 3 * DOWNLOAD_WORDS, "no longer three trips"
    assert at[1] < DOWNLOAD_WORDS < at[1] + ns[1], "the first boundary no longer falls inside column 1"
    assert at[3] < 2 * DOWNLOAD_WORDS and at[4] - 2 * DOWNLOAD_WORDS == 4, "column 3 no longer ends four words into the third trip"
    check_host_trees(ctx, host_trees, names)


def test_host_trees_with_a_column_that_starts_on_a_chunk_boundary(ctx, host_trees):
    names = ["23", "22a", "11"]
    ns = [len(host_trees[x][0]) for x in names]
    at = packed_offsets(ns)
    assert at[1] == DOWNLOAD_WORDS, "column 1 no longer starts on the first boundary"
    assert DOWNLOAD_WORDS < at[2] and at[3] <= 2 * DOWNLOAD_WORDS, "columns 1 and 2 no longer share the second trip"
    check_host_trees(ctx, host_trees, names)


# ---------------------------------------------------------------- 3: the prover against G.prove, word for word
# 16: five device layers (j = 11 .. 15); 20: nine; 22: layers 20 and 21 read a `hi` weight stage of 2^(j - 11) >= 1024 words
FS_SIZES = [16, 17, 20, 22]
FIXED_SIZES = [17, 21]
MIXED_PROOFS = [17, 12, 19, 15, 1, 18]


def proof_of(c, ch=None):
    p = G.prove(c, ch)
    assert int(p[0]) != 0
    return p


@pytest.fixture(scope="module")
def fs_proofs():
    """v -> the Fiat-Shamir proof of col(v)"""
    return {v: proof_of(col(v)) for v in sorted(set(FS_SIZES + MIXED_PROOFS))}


@pytest.mark.parametrize("v", FS_SIZES)
def test_prover_equals_the_reference(ctx, fs_proofs, v):
    got, = prove_dev(ctx, [col(v)])
    assert G.same(got, fs_proofs[v])
    assert got[0] == product(col(v))


@pytest.mark.parametrize("v", FIXED_SIZES)
def test_prover_with_fixed_edge_challenges_equals_the_reference(ctx, v):
    ch = G.edge_challenges(v, seed=v)
    got, = prove_dev(ctx, [col(v)], [ch])
    assert G.same(got, proof_of(col(v), ch))


def test_prover_host_form_equals_the_reference(ctx, fs_proofs):
    got, = ctx.grand_product_prove_batch([col(20)])
    assert G.same(got, fs_proofs[20])


def test_prover_on_a_mixed_tall_batch_reversed_and_again(ctx, fs_proofs):
    """Four tall columns of different heights: the `who` subset of the per-layer runs has 4 members at j = 12 .. 14, then 3, 3, 2
    and 1 at j = 15 .. 18, and with the order reversed other instances of the batch.  Then fixed challenges per instance, each
    at its own offset (foff, fixed_at(j)) of the flat array"""
    assert [sum(v > j for v in MIXED_PROOFS) for j in range(11, 19)] == [5, 4, 4, 4, 3, 3, 2, 1]
    for order in (MIXED_PROOFS, MIXED_PROOFS[::-1], MIXED_PROOFS):
        got = prove_dev(ctx, [col(v) for v in order])
        for g, v in zip(got, order):
            assert G.same(g, fs_proofs[v]), v
    chs = [G.edge_challenges(v, seed=3) for v in MIXED_PROOFS]
    got = prove_dev(ctx, [col(v) for v in MIXED_PROOFS], chs)
    for g, v, ch in zip(got, MIXED_PROOFS, chs):
        assert G.same(g, proof_of(col(v), ch)), v


@pytest.fixture(scope="module")
def many_proofs():
    which, cols = many_columns([11, 12, 13], 8, 6)
    return which, cols, [proof_of(c) for c in cols]


def test_prover_on_4096_instances(ctx, many_proofs):
    """ZIGZ_BATCH_MAX instances: one tops hand-off of 4096 workgroups against one completion count, 4096 host walks, and the
    per-layer runs over every instance taller than 2^11 (j = 11: 2736 of them) and 2^12 (j = 12: 1377)"""
    which, cols, want = many_proofs
    ins = [cols[w] for w in which]
    assert [sum(len(c) > 1 << j for c in ins) for j in (11, 12, 13)] == [2736, 1377, 0]
    d = Dev(ctx, ins)
    try:
        got = ctx.dev_grand_product_prove_batch(d.ptrs, [len(c) for c in ins])
        back, at = whole(ctx, d, ins)
        assert all(np.array_equal(back[a: a + len(c)], c) for a, c in zip(at, ins)), "a column was written"
    finally:
        d.free()
    assert len(got) == BATCH_MAX
    bad = [i for i, (g, w) in enumerate(zip(got, which)) if not G.same(g, want[w])]
    assert not bad, "%d proofs differ, the first at %d (2^%d)" % (len(bad), bad[0], len(ins[bad[0]]).bit_length() - 1)


@pytest.mark.parametrize("kind", G.COLUMN_KINDS)
def test_prover_on_the_column_kinds_at_2_to_the_16(ctx, kind):
    """two fused passes and five device layers over the saturated columns as well"""
    c = G.column(kind, 16, seed=11)
    if kind == "random":
        assert c.all()
    got, = prove_dev(ctx, [c])
    want = G.prove(c)
    assert (int(want[0]) == 0) == (kind == "one_zero")
    assert G.same(got, want)


# ---------------------------------------------------------------- 4: the verifier
def test_verifier_accepts_the_honest_tall_proofs(ctx, fs_proofs):
    sizes = [20, 22]
    cols, proofs = [col(v) for v in sizes], [fs_proofs[v] for v in sizes]
    for verd, exp, orc, rej in (verify_dev(ctx, cols, proofs), ctx.grand_product_verify_batch(cols, proofs)):
        assert list(verd) == [1, 1] and rej == 0
        assert exp == [int(p[6]) for p in proofs] and orc == exp


def test_verifier_rejects_every_tamper_at_2_to_the_17(ctx):
    c, proof = G.pinned(17)
    assert int(proof[0]) != 0
    t = G.tampered(c, proof)
    names = list(G.TAMPERS)
    cols = [c] + [t[x][0] for x in names]
    proofs = [proof] + [t[x][1] for x in names]
    want = [G.verdict(a, b) for a, b in zip(cols, proofs)]
    assert want[0][0] and not any(w[0] for w in want[1:])
    for verd, exp, orc, rej in (verify_dev(ctx, cols, proofs), ctx.grand_product_verify_batch(cols, proofs)):
        assert [bool(x) for x in verd] == [w[0] for w in want] and rej == len(names)
        assert exp == [w[1] for w in want], [n for n, a, w in zip(["honest"] + names, exp, want) if a != w[1]]
        assert orc == [w[2] for w in want]
    # the deferred form: the same replays without the column, whose change is then the caller's to notice
    want = [G.verdict(a, b, leaf_deferred=True) for a, b in zip(cols, proofs)]
    assert [w[0] for w in want] == [True] + [x == "column" for x in names]
    ns = [len(c)] * len(cols)
    for verd, exp, orc, rej in (ctx.dev_grand_product_verify_batch(None, ns, proofs, DEFERRED),
                                ctx.grand_product_verify_batch(None, proofs, DEFERRED, ns=ns)):
        assert [bool(x) for x in verd] == [w[0] for w in want] and rej == len(names) - 1
        assert exp == [w[1] for w in want] and orc == [None] * len(cols)


# ---------------------------------------------------------------- 5: one context
# The grand product carves the zero-check family's three workspaces and pinned region through sched::ZeroCheck and adds WS_GP,
# WS_GP_IN, WS_GP_TREE, a staging region and the tops' hand-off.  Calls of every family on ONE context, one behind the other; F is
# the one-context test of the other families, whose instances and calls are reused.
GP_FIRST = [10, 15, 12, 11]
GP_LARGER = [13, 15, 14, 15, 11, 12, 10, 14]
assert sum(1 << v for v in GP_LARGER) > sum(1 << v for v in GP_FIRST) and len(GP_LARGER) > len(GP_FIRST)


def gp_columns(sizes, seed):
    return [col(v, seed + i) for i, v in enumerate(sizes)]


def gp_prove(ctx, dev, cols, chs):
    return prove_dev(ctx, cols, chs) if dev else ctx.grand_product_prove_batch(cols, chs)


def gp_first(ctx, dev):
    return gp_prove(ctx, dev, gp_columns(GP_FIRST, 40), None)


def gp_larger(ctx, dev):
    return gp_prove(ctx, dev, gp_columns(GP_LARGER, 50), [G.edge_challenges(v, seed=7 + i) for i, v in enumerate(GP_LARGER)])


def gp_layers(ctx, dev):
    cols = gp_columns(GP_LARGER[:5], 60)
    return dev_layers(ctx, cols) if dev else ctx.product_layers_batch(cols)


@pytest.fixture(scope="module")
def verify_case():
    """the columns of the first call with their reference proofs, one of them with a changed round"""
    cols = gp_columns(GP_FIRST, 40)
    proofs = [proof_of(c) for c in cols]
    return cols, proofs, proofs[:2] + [G.tampered(cols[2], proofs[2])["round"][1]] + proofs[3:]


def one_context_calls(verify_case):
    cols, _, mixed = verify_case

    def gp_verify(ctx, dev):
        return verify_dev(ctx, cols, mixed) if dev else ctx.grand_product_verify_batch(cols, mixed)

    return [
        ("grand product", gp_first),
        ("zero-check", lambda ctx, dev: F.prove(ctx, 1, dev)),
        ("product layers", gp_layers),
        ("sum of products", lambda ctx, dev: F.prove(ctx, 2, dev)),
        ("grand product, larger", gp_larger),
        ("grand product verify", gp_verify),
        ("product", lambda ctx, dev: F.prove(ctx, 4, dev)),
        ("grand product again", gp_first),
    ]


@pytest.mark.parametrize("dev", [True, False], ids=["device_forms", "host_forms"])
def test_every_call_equals_the_same_call_on_a_fresh_context(verify_case, dev):
    import zigz_amd
    assert F.CALLS[1][0] == "zerocheck" and F.CALLS[2][0] == "sop" and F.CALLS[4][0] == "product"
    calls = one_context_calls(verify_case)
    want = []
    for _, call in calls:
        with zigz_amd.Context(0) as fresh:
            want.append(call(fresh, dev))
    with zigz_amd.Context(0) as ctx:
        got = [call(ctx, dev) for _, call in calls]
    for (name, _), g, w in zip(calls, got, want):
        assert F.same(g, w), name
    assert F.same(got[0], got[7])
    # ... and they are the reference's: the first call's proofs, the verdicts on them
    _, proofs, _ = verify_case
    assert len(got[0]) == len(proofs) and all(G.same(g, w) for g, w in zip(got[0], proofs))
    assert list(got[5][0]) == [1, 1, 0, 1] and got[5][3] == 1
