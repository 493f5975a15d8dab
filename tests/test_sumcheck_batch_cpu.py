"""The batched radix sumcheck schedule on the CPU: zigz_sumcheck_radix_run_batch (the orchestration behind
zigz_dev_sumcheck_prove_batch / zigz_sumcheck_prove_batch / zigz_lasso_prove_batch) over numpy stand-in data passes.
Every table of a batch must give the bytes of its own SumcheckProver.prove, with and without fixed challenges."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O

P = O.P_BB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 4, 1024, 2048, 1 << 12, 1 << 13, 1 << 15, 1 << 17]
NEW_SYMBOLS = ["zigz_dev_sumcheck_prove_batch", "zigz_sumcheck_prove_batch", "zigz_lasso_prove_batch",
               "zigz_sumcheck_radix_run_batch"]


class NumpyBatchOps:
    """The three batched passes on numpy tables (exact: products reduced mod p before they are summed, sums < 2^41)."""

    def __init__(self, tables):
        self.t = [np.asarray(t, dtype=np.uint64).copy() for t in tables]
        self.calls = []

    @staticmethod
    def _block_sums(t, k):
        return [int(x) for x in t.reshape(1 << k, -1).sum(axis=1, dtype=np.uint64)]

    def block_sums(self, tables, ks):
        self.calls.append(("block_sums", list(tables)))
        return [self._block_sums(self.t[i], k) for i, k in zip(tables, ks)]

    def fold(self, tables, ks, weights, k_next):
        self.calls.append(("fold", list(tables)))
        out = []
        for i, k, w, kn in zip(tables, ks, weights, k_next):
            T = self.t[i].reshape(1 << k, -1)
            W = np.asarray(w, dtype=np.uint64)[:, None]
            self.t[i] = ((W * T) % np.uint64(P)).sum(axis=0, dtype=np.uint64) % np.uint64(P)
            out.append(self._block_sums(self.t[i], kn) if kn else None)
        return out

    def read_tail(self, tables, ms):
        self.calls.append(("read_tail", list(tables)))
        for i, m in zip(tables, ms):
            assert len(self.t[i]) == m
        return [[int(x) for x in self.t[i]] for i in tables]


def _batch(k, seed):
    rng = np.random.default_rng(seed)
    ns = [int(rng.choice(SIZES)) for _ in range(k)]
    if k > 1:
        ns[-1] = ns[0]  # a repeated size
    tables = [O.splitmix64_field(seed * 100 + i, n) for i, n in enumerate(ns)]
    return ns, tables


@pytest.mark.parametrize("k,seed", [(1, 1), (1, 2), (3, 3), (16, 4)])
@pytest.mark.parametrize("fixed", [False, True])
def test_radix_run_batch_matches_oracle(k, seed, fixed):
    from zigz_amd import shard
    ns, tables = _batch(k, seed)
    chs = [O.splitmix64_field(seed * 7 + i, n.bit_length() - 1) for i, n in enumerate(ns)] if fixed else None
    out = shard.sumcheck_radix_run_batch(NumpyBatchOps(tables), ns, challenges=chs)
    assert len(out) == k
    for i in range(k):
        r0, p0, fe0 = O.sumcheck_prove(P, tables[i], chs[i] if fixed else None)
        assert O.sumcheck_to_bytes(*out[i]) == O.sumcheck_to_bytes(r0, p0, fe0), (i, ns[i])


def test_radix_run_batch_every_size_and_the_same_table_twice():
    """every size of the list in one batch, one table twice: one block-sums pass, tables drop out, one tail hand-off"""
    from zigz_amd import shard
    ns = SIZES + [1 << 17]
    tables = [O.splitmix64_field(500 + i, n) for i, n in enumerate(SIZES)]
    tables.append(tables[-1])
    ops = NumpyBatchOps(tables)
    out = shard.sumcheck_radix_run_batch(ops, ns)
    for i in range(len(ns)):
        assert O.sumcheck_to_bytes(*out[i]) == O.sumcheck_to_bytes(*O.sumcheck_prove(P, tables[i]))
    assert out[-1][2] == out[-2][2]
    kinds = [c[0] for c in ops.calls]
    assert kinds[0] == "block_sums" and kinds[-1] == "read_tail" and kinds.count("block_sums") == 1 and kinds.count("read_tail") == 1
    assert ops.calls[0][1] == [i for i, n in enumerate(ns) if n > 1024]  # the small tables go straight to the tail
    assert ops.calls[-1][1] == list(range(len(ns)))                      # every tail in one hand-off
    # a table leaves the folds once it is down to <= 1024 entries: every fold serves a subset of the one before
    folds = [c[1] for c in ops.calls if c[0] == "fold"]
    assert all(set(b) <= set(a) for a, b in zip(folds, folds[1:]))


@pytest.mark.parametrize("where", ["block_sums", "fold", "read_tail"])
def test_radix_run_batch_pass_error_is_returned(where):
    from zigz_amd import shard, errors

    class Broken(NumpyBatchOps):
        pass

    def fail(*a):
        return 101  # ZIGZ_ERR_HIP

    ops = Broken([O.splitmix64_field(9, 1 << 12), O.splitmix64_field(10, 4)])
    setattr(ops, where, fail)
    with pytest.raises(errors.ZigzError) as e:
        shard.sumcheck_radix_run_batch(ops, [1 << 12, 4])
    assert e.value.code == 101


def test_radix_run_batch_argument_errors():
    from zigz_amd import shard, errors
    ops = NumpyBatchOps([O.splitmix64_field(1, 8)] * 3)
    assert shard.sumcheck_radix_run_batch(ops, []) == []
    for ns, code in [([8, 6, 8], errors.LENGTH_NOT_POWER_OF_TWO), ([8, 1, 8], errors.NO_VARIABLES),
                     ([8, 0, 8], errors.EMPTY_EVALUATIONS)]:
        with pytest.raises(errors.ZigzError) as e:
            shard.sumcheck_radix_run_batch(ops, ns)
        assert e.value.code == code
    with pytest.raises(errors.ZigzError) as e:
        shard.sumcheck_radix_run_batch(ops, [8, 8], challenges=[[1, 2, 3], [1, P, 3]])
    assert e.value.code == errors.NOT_CANONICAL


def test_batch_symbols_declared_exported_and_typed():
    from zigz_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    assert re.search(r"#define ZIGZ_BATCH_MAX 4096\b", hdr)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _ffi.SIGNATURES, name
        assert getattr(_ffi.lib, name) is not None
    for cb in ["zigz_radix_batch_sums_fn", "zigz_radix_batch_fold_fn", "zigz_radix_batch_tail_fn"]:
        assert re.search(r"typedef zigz_status \(\*%s\)\(" % cb, hdr), cb
