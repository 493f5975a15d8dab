"""The product, zero-check and sum-of-products provers on ONE context, one behind the other: they run one round schedule
(product_schedule.hpp) over the same three workspaces and the same pinned region, which each family carves in its own way.  Every
call's result equals, word for word, the same call on a context of its own -- so no family's layout depends on what the call before
it left behind.  Challenges are fixed, so the comparison is exact.

The order: product, zero-check, sop, zero-check with a larger batch (more descriptors, weights and partials than the first, so every
region behind them moves), product.  The batches mix n = 2^10 (host only), 2^11 (round 0, then one bind pass whose sums nobody
reads), 2^12 and 2^13; the pools have 1, 3 and 8 tables, 1 and 8 terms of degree 1 to 3."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

P = O.P_BB


def rnd(seed, n):
    return O.splitmix64_field(seed, n)


def terms_of(M, T, seed):
    """T terms over a pool of M tables whose degrees cycle through 1, 2, 3 (a single term is cubic)"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, P)), tuple(int(rng.integers(0, M)) for _ in range(3 if T == 1 else 1 + t % 3))) for t in range(T)]


def product_batch(seed):
    shapes = [(1, 10), (2, 11), (3, 12), (1, 13), (3, 11), (2, 13)]  # (d, log2 n)
    return [[rnd(seed + 10 * i + j, 1 << v) for j in range(d)] for i, (d, v) in enumerate(shapes)]


def pool_batch(seed, shapes, with_tau):
    """shapes: (M, T, log2 n) per instance -> (tables, terms[, tau])"""
    out = []
    for i, (M, T, v) in enumerate(shapes):
        inst = ([rnd(seed + 10 * i + j, 1 << v) for j in range(M)], terms_of(M, T, seed + i))
        out.append(inst + ([int(x) for x in rnd(seed + 10 * i + 9, v)],) if with_tau else inst)
    return out


SMALL = [(1, 1, 11), (3, 8, 12)]
LARGE = [(1, 8, 10), (3, 1, 11), (8, 8, 12), (8, 1, 13), (3, 8, 13), (1, 1, 12), (8, 8, 11)]
assert sum(M * (1 << v) for M, _, v in LARGE if v > 10) > sum(M * (1 << v) for M, _, v in SMALL)

# (family, instances) in the order they are called
CALLS = [
    ("product", product_batch(31000)),
    ("zerocheck", pool_batch(32000, SMALL, True)),
    ("sop", pool_batch(33000, LARGE[:5], False)),
    ("zerocheck", pool_batch(34000, LARGE, True)),
    ("product", product_batch(35000)),
]


def tables_of(family, inst):
    return inst if family == "product" else inst[0]


def challenges_of(call, family, instances):
    return [rnd(36000 + 100 * call + i, len(tables_of(family, inst)[0]).bit_length() - 1) for i, inst in enumerate(instances)]


def prove(ctx, call, dev):
    family, instances = CALLS[call]
    ch = challenges_of(call, family, instances)
    if not dev:
        return getattr(ctx, f"sumcheck_prove_{family}_batch")(instances, ch)
    bufs = []
    try:
        d_instances = []
        for inst in instances:
            ptrs = []
            for t in tables_of(family, inst):
                bufs.append(ctx.dev_alloc(4 * len(t)))
                ctx.upload(t, bufs[-1])
                ptrs.append(bufs[-1])
            d_instances.append(ptrs if family == "product" else (ptrs,) + tuple(inst[1:]))
        ns = [len(tables_of(family, inst)[0]) for inst in instances]
        return getattr(ctx, f"dev_sumcheck_prove_{family}_batch")(d_instances, ns, ch)
    finally:
        for b in bufs:
            ctx.dev_free(b)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))


@pytest.mark.parametrize("dev", [True, False], ids=["device_forms", "host_forms"])
def test_every_call_equals_the_same_call_on_a_fresh_context(dev):
    import zigz_amd
    want = []
    for call in range(len(CALLS)):
        with zigz_amd.Context(0) as fresh:
            want.append(prove(fresh, call, dev))
    with zigz_amd.Context(0) as ctx:
        got = [prove(ctx, call, dev) for call in range(len(CALLS))]
    for call, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(CALLS[call][1]) and same(g, w), f"call {call} ({CALLS[call][0]})"
    # the proofs are no constants: the two product calls and the two zero-check calls differ
    assert not same(got[0], got[4]) and not same(got[1][0], got[3][0])
