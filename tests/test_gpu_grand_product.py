"""Product trees and the batched grand-product argument on the GPU (zigz_[dev_]product_layers_batch,
zigz_[dev_]grand_product_prove_batch, zigz_[dev_]grand_product_verify_batch): every comparison is exact, word for word -- the trees
against numpy, the proofs against grand_product_ref.py up to 2^14 and, layer by layer, against the existing closed-form zero-check
entry at 2^17 and 2^20, the verdicts against the reference's."""
import numpy as np
import pytest

import grand_product_ref as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB
_P = np.uint64(P)
E = None
DEFERRED = 1  # ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED
GUARD = 0x5A5A5A5  # a canonical word no tree of the tests holds
GUARD_WORDS = 8


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


class Dev:
    """host columns uploaded one behind the other into one device buffer, each 16-byte aligned"""

    def __init__(self, ctx, tables):
        self.ctx = ctx
        offs, o = [], 0
        for t in tables:
            offs.append(o)
            o += (len(t) + 3) // 4 * 4
        self.base = ctx.dev_alloc((o + 4) * 4)
        packed = np.zeros(o, dtype=np.uint64)
        for t, a in zip(tables, offs):
            packed[a: a + len(t)] = t
        ctx.upload(packed, self.base)
        self.ptrs = [self.base + 4 * a for a in offs]

    def free(self):
        self.ctx.dev_free(self.base)


def col(v, seed=0):
    return O.splitmix64_field(23000 + 37 * v + seed, 1 << v)


def product(c):
    """the numpy reduction: halves multiplied until one word is left"""
    c = np.asarray(c, dtype=np.uint64)
    while len(c) > 1:
        c = (c[:len(c) // 2] * c[len(c) // 2:]) % _P
    return int(c[0])


def dev_layers(ctx, cols):
    """the device form over guarded output buffers: returns the n words of every buffer after checking that the guard words behind
    it and its word n - 1 are untouched and that the caller's columns are unchanged"""
    d = Dev(ctx, cols)
    outs = Dev(ctx, [np.full(len(c) + GUARD_WORDS, GUARD, dtype=np.uint64) for c in cols])
    try:
        ctx.dev_product_layers_batch(d.ptrs, [len(c) for c in cols], outs.ptrs)
        got = []
        for c, p in zip(cols, outs.ptrs):
            w = ctx.download(p, len(c) + GUARD_WORDS)
            assert np.all(w[len(c) - 1:] == GUARD), "word n - 1 or a guard word behind the buffer was written"
            got.append(w[:len(c)])
        for c, p in zip(cols, d.ptrs):
            assert np.array_equal(ctx.download(p, len(c)), c)
        return got
    finally:
        d.free()
        outs.free()


# ---------------------------------------------------------------- 1: the trees
# 2, 3, 11: only k_gp_top; 12: one fused level, then the top; 13: two levels; 14: one full three-level pass; 15: three plus one; 17:
# two passes
TREE_SIZES = [2, 3, 11, 12, 13, 14, 15, 17]


@pytest.fixture(scope="module")
def tree_cases():
    cols = [col(v) for v in TREE_SIZES]
    return cols, [G.tree_buffer(c, fill=GUARD) for c in cols]


@pytest.mark.parametrize("i", range(len(TREE_SIZES)), ids=["v%d" % v for v in TREE_SIZES])
def test_layers_equal_numpy(ctx, tree_cases, i):
    cols, want = tree_cases
    got, = dev_layers(ctx, [cols[i]])
    assert np.array_equal(got, want[i])
    assert int(got[len(got) - 2]) == product(cols[i])


def test_layers_of_a_mixed_batch_and_its_reverse(ctx, tree_cases):
    cols, want = tree_cases
    for order in (list(range(len(cols))), list(range(len(cols)))[::-1]):
        got = dev_layers(ctx, [cols[i] for i in order])
        for g, i in zip(got, order):
            assert np.array_equal(g, want[i]), TREE_SIZES[i]


def test_layers_host_form_and_edge_columns(ctx):
    cols = [G.column(kind, 13, seed=3) for kind in G.COLUMN_KINDS] + [col(1), col(12, 5)]
    got = ctx.product_layers_batch(cols)
    for g, c in zip(got, cols):
        assert np.array_equal(g, G.tree_buffer(c, fill=0))


# ---------------------------------------------------------------- 2: the prover against the reference, word for word
def prove_dev(ctx, cols, challenges=None):
    d = Dev(ctx, cols)
    try:
        out = ctx.dev_grand_product_prove_batch(d.ptrs, [len(c) for c in cols], challenges)
        for c, p in zip(cols, d.ptrs):
            assert np.array_equal(ctx.download(p, len(c)), c)
        return out
    finally:
        d.free()


@pytest.mark.parametrize("fixed", [False, True], ids=["fiat_shamir", "fixed_edge"])
@pytest.mark.parametrize("v", [1, 2, 11, 12, 13, 14])
def test_prover_equals_the_reference(ctx, v, fixed):
    c = col(v, 1)
    ch = G.edge_challenges(v, seed=v) if fixed else None
    got, = prove_dev(ctx, [c], None if ch is None else [ch])
    assert G.same(got, G.prove(c, ch))
    if not fixed:
        assert got[0] == product(c)


@pytest.mark.parametrize("kind", G.COLUMN_KINDS)
def test_prover_on_the_column_kinds_at_2_to_the_12(ctx, kind):
    c = G.column(kind, 12, seed=7)
    want = G.prove(c)
    got, = prove_dev(ctx, [c])
    assert G.same(got, want)
    ch = G.edge_challenges(12, seed=len(kind))
    got, = prove_dev(ctx, [c], [ch])
    assert G.same(got, G.prove(c, ch))


@pytest.fixture(scope="module")
def mixed():
    cols = [col(v, 2) for v in (1, 5, 11, 12, 14)]
    return cols, [G.prove(c) for c in cols]


def test_prover_on_a_mixed_batch_reversed_and_again(ctx, mixed):
    cols, want = mixed
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [0, 1, 2, 3, 4]):
        got = prove_dev(ctx, [cols[i] for i in order])
        for g, i in zip(got, order):
            assert G.same(g, want[i]), len(cols[i])
    ch = [G.edge_challenges(len(c).bit_length() - 1, seed=3) for c in cols]
    got = prove_dev(ctx, cols, ch)
    for g, c, x in zip(got, cols, ch):
        assert G.same(g, G.prove(c, x))


# ---------------------------------------------------------------- 3: the prover against the existing zero-check entry, layer by layer
@pytest.mark.parametrize("v", [17, 20])
def test_prover_equals_the_zerocheck_entry_layer_by_layer(ctx, v):
    """Every layer j >= 1 of a Fiat-Shamir proof is the existing entry's proof of the two halves of layer j + 1 taken from the layers
    entry's buffer, under the proof's tau^(j), with the layer's points as fixed challenges: the same rounds, table_evals = (l_j, h_j),
    claimed sum = the carried claim.  All layers run as ONE batch of the existing entry.  (Layer 1's H half starts 8 bytes into a
    16-byte vector, which the device form does not take: that layer goes through the entry's host form.)"""
    n = 1 << v
    c = col(v, 4)
    d = Dev(ctx, [c])
    tree = ctx.dev_alloc(4 * n)
    try:
        proof, = ctx.dev_grand_product_prove_batch(d.ptrs, [n])
        product_, evals, rounds, points, chs, leaf, leaf_eval = proof
        assert product_ == product(c)
        ctx.dev_product_layers_batch(d.ptrs, [n], [tree])
        buf = ctx.download(tree, n)
        assert int(buf[n - 2]) == product_
        # the carried claims and taus, from the proof's own words
        tau, claim, taus, claims = [], product_, [], []
        for j in range(v):
            taus.append(list(tau))
            claims.append(claim)
            q = [int(x) for x in points[j * (j - 1) // 2: j * (j - 1) // 2 + j]][::-1]
            lj, hj, cj = int(evals[2 * j]), int(evals[2 * j + 1]), int(chs[j])
            tau, claim = q + [cj], (lj + cj * (hj - lj)) % P
        assert [int(x) for x in leaf] == tau and leaf_eval == claim
        assert int(evals[0]) * int(evals[1]) % P == product_
        term = [(1, (0, 1))]

        def check(j, got):
            claimed, r, pt, te, _, _ = got
            assert np.array_equal(r, rounds[2 * j * (j - 1): 2 * j * (j + 1)]), j
            assert np.array_equal(pt, points[j * (j - 1) // 2: j * (j - 1) // 2 + j])
            assert [int(x) for x in te] == [int(evals[2 * j]), int(evals[2 * j + 1])], j
            assert claimed == claims[j], j

        got, = ctx.sumcheck_prove_zerocheck_batch([([buf[n - 8: n - 6], buf[n - 6: n - 4]], term, taus[1])], [points[0:1]])  # V_2 = L_1 | H_1
        check(1, got)
        inst, ns, chal = [], [], []
        for j in range(2, v):
            nxt = d.ptrs[0] if j + 1 == v else tree + 4 * (n - (2 << (j + 1)))
            inst.append(([nxt, nxt + 4 * (1 << j)], term, taus[j]))
            ns.append(1 << j)
            chal.append(points[j * (j - 1) // 2: j * (j - 1) // 2 + j])
        for j, got in zip(range(2, v), ctx.dev_sumcheck_prove_zerocheck_batch(inst, ns, chal)):
            check(j, got)
    finally:
        ctx.dev_free(tree)
        d.free()


# ---------------------------------------------------------------- 4: the verifier
def verify_dev(ctx, cols, proofs, flags=0):
    d = Dev(ctx, cols)
    try:
        return ctx.dev_grand_product_verify_batch(d.ptrs, [len(c) for c in cols], proofs, flags)
    finally:
        d.free()


def test_verifier_accepts_honest_proofs_on_every_form(ctx, mixed):
    cols, want = mixed
    ns = [len(c) for c in cols]
    host_made = ctx.grand_product_prove_batch(cols)  # made on the host form ...
    for g, w in zip(host_made, want):
        assert G.same(g, w)
    for verd, exp, orc, rej in (verify_dev(ctx, cols, host_made), ctx.grand_product_verify_batch(cols, want)):  # ... verified on the device form
        assert list(verd) == [1] * len(cols) and rej == 0
        assert exp == [int(p[6]) for p in want] and orc == exp
    for verd, exp, orc, rej in (ctx.dev_grand_product_verify_batch(None, ns, want, DEFERRED),
                                ctx.grand_product_verify_batch(None, want, DEFERRED, ns=ns)):
        assert list(verd) == [1] * len(cols) and rej == 0 and exp == [int(p[6]) for p in want] and orc == [None] * len(cols)


def test_verifier_rejects_every_tamper_at_2_to_the_12(ctx):
    c, proof = G.pinned(12)
    t = G.tampered(c, proof)
    names = list(G.TAMPERS)
    cols = [c] + [t[x][0] for x in names]
    proofs = [proof] + [t[x][1] for x in names]
    want = [G.verdict(a, b) for a, b in zip(cols, proofs)]
    assert want[0][0] and not any(w[0] for w in want[1:])
    for verd, exp, orc, rej in (verify_dev(ctx, cols, proofs), ctx.grand_product_verify_batch(cols, proofs)):
        assert list(verd) == [1] + [0] * len(names) and rej == len(names)
        assert exp == [w[1] for w in want], [n for n, a, w in zip(["honest"] + names, exp, want) if a != w[1]]
        assert orc == [w[2] for w in want]
    # without the column a changed leaf is the caller's to notice; everything else is still rejected
    verd, exp, orc, rej = ctx.dev_grand_product_verify_batch(None, [len(c)] * len(cols), proofs, DEFERRED)
    assert list(verd) == [1] + [int(x == "column") for x in names] and rej == len(names) - 1
    assert exp == [G.verdict(a, b, leaf_deferred=True)[1] for a, b in zip(cols, proofs)]


def test_flags_and_statuses(ctx, mixed):
    cols, want = mixed
    ns = [len(c) for c in cols]
    assert ctx.dev_grand_product_prove_batch([], []) == [] and ctx.grand_product_prove_batch([]) == []
    ctx.dev_product_layers_batch([], [], [])
    assert ctx.dev_grand_product_verify_batch([], [], [])[3] == 0
    d = Dev(ctx, cols)
    try:
        cases = [
            (lambda: ctx.dev_grand_product_verify_batch(d.ptrs, ns, want, DEFERRED), "INVALID_ARGUMENT", None),
            (lambda: ctx.dev_grand_product_verify_batch(None, ns, want, 0), "INVALID_ARGUMENT", None),
            (lambda: ctx.dev_grand_product_verify_batch(d.ptrs, ns, want, 2), "INVALID_ARGUMENT", None),
            (lambda: ctx.dev_grand_product_prove_batch([d.ptrs[0], d.ptrs[1] + 8], ns[:2]), "INVALID_ARGUMENT", 1),
            (lambda: ctx.dev_grand_product_prove_batch(d.ptrs[:3], [2, 32, 1]), "NO_VARIABLES", 2),
            (lambda: ctx.dev_grand_product_prove_batch(d.ptrs[:3], [2, 24, 2048]), "LENGTH_NOT_POWER_OF_TWO", 1),
            (lambda: ctx.dev_product_layers_batch(d.ptrs[:2], [2, 0], d.ptrs[2:4]), "EMPTY_EVALUATIONS", 1),
            (lambda: ctx.dev_product_layers_batch(d.ptrs[:2], [2, 32], [d.ptrs[2], d.ptrs[3] + 4]), "INVALID_ARGUMENT", 1),
            (lambda: ctx.dev_grand_product_prove_batch(d.ptrs[:2], ns[:2], [[0], [P] * 15]), "NOT_CANONICAL", 1),
        ]
        for call, name, idx in cases:
            with pytest.raises(E.ZigzError) as e:
                call()
            assert e.value.code == getattr(E, name) and (idx is None or e.value.bad_index == idx), name
    finally:
        d.free()
    bad = [cols[1].copy(), cols[3].copy()]
    bad[1][4000] = P
    for call in (lambda: ctx.grand_product_prove_batch(bad), lambda: ctx.product_layers_batch(bad),
                 lambda: ctx.grand_product_verify_batch(bad, [want[1], want[3]])):
        with pytest.raises(E.ZigzError) as e:
            call()
        assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    worse = list(want[3])
    worse[2] = worse[2].copy()
    worse[2][7] = P  # a proof word >= p is an argument error, not a rejection
    with pytest.raises(E.ZigzError) as e:
        ctx.grand_product_verify_batch([cols[1], cols[3]], [want[1], tuple(worse)])
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
