"""Exact, DEDUPLICATING host reference of SimpleMerkleTree (merkle_tree.zig as restated in oracle/zigz_oracle.c), numpy and
hashlib only -- no zigz_amd, no C oracle:

    leaf  = SHA3-256(value as 8 little-endian bytes)      leaves beyond n are hashLeaf(0)
    node  = SHA3-256(left || right)                       npad = the next power of two of n

The C oracle hashes every node (2^27 permutations for one 2^26 column: minutes).  This reference hashes every DISTINCT leaf
value once and, level by level, every distinct (left, right) pair once: per level it keeps one small integer id per node --
equal ids <=> equal subtrees (equal leaf values below) -- and one digest per id.  For the columns the structure-aware
builds are made for (loops, piecewise-constant runs) that is a few thousand hashes and seconds at 2^26, and it gives the
root, every opening path and exact counts of the nodes that differ.  tests/test_merkle_ref_cpu.py pins it to the C oracle.

Also here: the numpy model of the run-aware leader rule (which nodes k_runs_stage hashes), used by the GPU tests."""
import hashlib

import numpy as np

_LUT_SPACE = 1 << 22   # key spaces up to this size are factorised through a lookup table
_SAMPLE_MIN = 1 << 16  # longer key arrays try a strided sample of their keys before sorting everything


def _narrow(ids, count):
    """ids in the smallest unsigned type that holds `count` of them (2^26 nodes per level, up to 20 levels, many columns)"""
    return ids.astype(np.uint8 if count <= 1 << 8 else np.uint16 if count <= 1 << 16 else np.uint32)


def _factorize(keys, space):
    """(distinct keys ascending, id of every key = its position among them); keys are int64 in [0, space).
    Three ways to the same result: a table over the key space where that is small; the distinct keys of a strided sample,
    completed by whatever the sample missed (runs and loops are seen whole by a sample; sorting 2^26 keys is what costs);
    numpy's sort-based unique for the rest."""
    if space <= _LUT_SPACE:
        seen = np.zeros(space, dtype=bool)
        seen[keys] = True
        uniq = np.flatnonzero(seen)
        lut = np.cumsum(seen, dtype=np.int64) - 1
        return uniq, _narrow(lut[keys], uniq.size)
    if keys.size > _SAMPLE_MIN:
        cand = np.unique(keys[::61])
        if cand.size <= keys.size // 64:
            pos = np.minimum(np.searchsorted(cand, keys), cand.size - 1)
            miss = cand[pos] != keys
            n_miss = int(np.count_nonzero(miss))
            if n_miss == 0:
                return cand, _narrow(pos, cand.size)
            if n_miss <= keys.size // 16:
                cand = np.union1d(cand, keys[miss])  # now every key is in it, and everything in it is a key
                return cand, _narrow(np.searchsorted(cand, keys), cand.size)
    uniq, inv = np.unique(keys, return_inverse=True)
    return uniq, _narrow(inv.reshape(-1), uniq.size)


def _structure(leaf_keys, space):
    """ids of every level of the tree over the given leaf keys (a power of two of them), bottom-up.  Yields per level
    (ids, keys): ids[i] of node i, and per id what it was made of -- the leaf key (level 0) or left id * K + right id with
    K the number of ids of the level below."""
    uniq, ids = _factorize(leaf_keys, space)
    yield ids, uniq
    while ids.size > 1:
        k = int(uniq.size)
        pair = ids[0::2].astype(np.int64) * k + ids[1::2]
        uniq, ids = _factorize(pair, k * k)
        yield ids, uniq


def _padded(values, n):
    a = np.asarray(values).reshape(-1)
    n = a.size if n is None else int(n)
    assert 1 <= n <= a.size
    assert a.size == 0 or int(a.max()) < 1 << 62
    npad = 1 << (n - 1).bit_length()
    leaves = np.zeros(npad, dtype=np.int64)  # padding leaves are hashLeaf(0): a leaf of value 0
    leaves[:n] = a[:n]
    return leaves, n, npad


class MerkleRef:
    """One column's tree.  root (32 bytes), height, n, npad, hashes (digests computed); ids[l] / digests[l] per level l =
    0 (leaves) .. height (root): ids[l][i] is the id of node i, digests[l][id] its 32 bytes."""

    def __init__(self, values, n=None):
        leaves, self.n, self.npad = _padded(values, n)
        self.height = self.npad.bit_length() - 1
        self.ids, self.digests = [], []
        self.hashes = 0
        sha3 = hashlib.sha3_256
        for ids, keys in _structure(leaves, int(leaves.max()) + 1):
            if not self.ids:
                self._leaf_values = keys  # id -> value
                out = b"".join(sha3(int(v).to_bytes(8, "little")).digest() for v in keys.tolist())
            else:
                below = self.digests[-1].tobytes()
                k = self.digests[-1].shape[0]
                out = b"".join(sha3(below[32 * a:32 * a + 32] + below[32 * b:32 * b + 32]).digest()
                               for a, b in zip((keys // k).tolist(), (keys % k).tolist()))
            self.hashes += keys.size
            self.ids.append(ids)
            self.digests.append(np.frombuffer(out, dtype=np.uint8).reshape(-1, 32))
        assert len(self.ids) == self.height + 1 and self.ids[-1].size == 1
        self.root = self.digests[-1][0].tobytes()

    def node(self, level, i):
        return self.digests[level][self.ids[level][i]].tobytes()

    def level(self, level):
        """all digests of a level, node by node: (npad >> level, 32) u8 (small trees only)"""
        return self.digests[level][self.ids[level]]

    def value(self, index):
        return int(self._leaf_values[self.ids[0][index]])

    def open(self, index):
        """SimpleMerkleTree.open: (siblings [height * 32 bytes, leaf level first], directions [height bytes, 1 = the node
        on the path is the right child], leaf value) -- the layout of oracle_lib.merkle_open and CommitJob.open_all"""
        index = int(index)
        assert 0 <= index < self.n  # (the padded leaves cannot be opened)
        sib, dirs, ci = [], bytearray(), index
        for l in range(self.height):
            sib.append(self.node(l, ci ^ 1))
            dirs.append(ci & 1)
            ci >>= 1
        return b"".join(sib), bytes(dirs), self.value(index)

    def distinct(self, level):
        """distinct nodes (subtrees) of the column on that level"""
        return int(self.digests[level].shape[0])


class GroupRef:
    """A set of columns of one length looked at as ONE column of tuples: distinct_tuples(level) is the number of nodes of
    that level that differ in at least one column from every earlier one -- what a kept content-addressed group hashes per
    column and level."""

    def __init__(self, cols, n=None):
        key, space = None, 1
        for col in cols:
            leaves, self.n, self.npad = _padded(col, n)
            uniq, ids = _factorize(leaves, int(leaves.max()) + 1)
            if key is None:
                key, space = ids.astype(np.int64), int(uniq.size)
            else:  # (tuple so far, this column) -> one id again
                u2, key = _factorize(key * int(uniq.size) + ids, space * int(uniq.size))
                key, space = key.astype(np.int64), int(u2.size)
        self.height = self.npad.bit_length() - 1
        self.counts = [int(keys.size) for _, keys in _structure(key, space)]

    def distinct_tuples(self, level):
        return self.counts[level]


# ---------------------------------------------------------------- the run-aware leader rule (kernels.hpp, k_runs_stage)
def _run_tile_nodes(N, l):
    """kernels.hpp run_tile_nodes: the nodes one segment of a stage covers at level l (its first node is always hashed)."""
    if l == 0:
        return 4096
    s = (l - 1) // 6
    n_in = N >> (6 * s)
    return min(4096, n_in) >> (l - 6 * s)


def _list_levels(nv):
    """the list-driven levels of a 2^nv tree: 0 .. nv - 8 (down to 256 nodes per column)"""
    return nv - 8 + 1


def _run_aware_hashed(cols, levels):
    """numpy model of k_runs_stage: nodes hashed (not copied from the left neighbour) on levels 0..levels-1; the first node
    of every tile (what one segment of a stage covers at that level) is always hashed."""
    total = 0
    for col in cols if isinstance(cols, (list, tuple)) else np.asarray(cols):
        uni = np.ones(col.size, dtype=bool)
        for l in range(levels):
            if l:
                half = col[(1 << (l - 1))::(1 << l)]
                uni = uni[0::2] & uni[1::2] & (col[::(1 << l)] == half)
            val = col[::(1 << l)]
            copy = np.zeros(val.size, dtype=bool)
            copy[1:] = uni[1:] & uni[:-1] & (val[1:] == val[:-1])
            copy[::_run_tile_nodes(col.size, l)] = False
            total += int((~copy).sum())
    return total
