"""tests/merkle_ref.py (the deduplicating Merkle reference and the model of the run-aware leader rule) pinned to the C oracle
and to brute force, before any GPU test relies on it."""
import numpy as np
import pytest

import merkle_ref as M
import oracle_lib as O

P = O.P_BB
SIZES = [1, 2, 3, 5, 255, 256, 257, 4096, 5000, (1 << 15) + 1]
KINDS = ["random", "constant", "loop", "runs"]


def _column(kind, n, seed=0):
    step = np.arange(n, dtype=np.uint64)
    if kind == "random":
        return O.splitmix64_field(100 + n + seed, n)
    if kind == "constant":
        return np.full(n, 77 + seed, dtype=np.uint64)
    if kind == "loop":
        return (0x1000 + 4 * (step % np.uint64(12 + seed))).astype(np.uint64)
    if kind == "runs":
        return np.repeat(O.splitmix64_field(7 + seed, n // 37 + 1), 37)[:n].astype(np.uint64)
    raise ValueError(kind)


def _open_indices(n):
    """first, second, the middle, the last values (the last one's neighbours are padding leaves where n is not a power of two)"""
    return sorted({0, min(1, n - 1), n // 2, max(n - 3, 0), max(n - 2, 0), n - 1})


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_root_levels_and_openings_equal_the_oracle(kind, n):
    col = _column(kind, n)
    ref = M.MerkleRef(col)
    root, h = O.merkle_build(col)
    assert (ref.root, ref.height) == (root, h)
    lv, h2 = O.merkle_levels(col)
    npad = 1 << (n - 1).bit_length()
    assert ref.npad == npad and h2 == h
    off = 0
    for l in range(h + 1):
        nl = npad >> l
        assert ref.level(l).tobytes() == lv[32 * off:32 * (off + nl)].tobytes(), l
        off += nl
    for i in _open_indices(n):
        assert ref.open(i) == O.merkle_open(col, i), i
        assert ref.value(i) == int(col[i])


def test_fewer_values_than_the_array_holds():
    col = _column("runs", 300)
    assert M.MerkleRef(col, n=257).root == O.merkle_build(col[:257])[0]
    assert M.MerkleRef(col, n=256).root == O.merkle_build(col[:256])[0]


def _brute_distinct(level_bytes):
    """distinct 32 * k byte rows"""
    return len({r.tobytes() for r in level_bytes})


@pytest.mark.parametrize("nv", [10, 11, 12])
def test_distinct_counts_equal_brute_force(nv):
    """distinct(level) per column and distinct_tuples(level) of a group equal counts over the oracle's digests: equal digests
    <=> equal subtrees, and a group's node is a new one when it differs from every earlier node in at least one column."""
    N = 1 << nv
    step = np.arange(N, dtype=np.uint64)
    cols = [(0x1000 + 4 * (step % np.uint64(12))), (step % np.uint64(12)) % np.uint64(5), np.zeros(N, dtype=np.uint64),
            step % np.uint64(3), np.repeat(O.splitmix64_field(nv, N // 64), 64), (step % np.uint64(31)) * np.uint64(7)]
    cols[1] = cols[1].copy()
    cols[1][N - 100:] = 0  # a tail that breaks the loop
    levels = []
    for c in cols:
        lv, h = O.merkle_levels(c)
        per, off = [], 0
        for l in range(h + 1):
            per.append(lv[32 * off:32 * (off + (N >> l))].reshape(N >> l, 32))
            off += N >> l
        levels.append(per)
    refs = [M.MerkleRef(c) for c in cols]
    for l in range(nv + 1):
        for r, per in zip(refs, levels):
            assert r.distinct(l) == _brute_distinct(per[l]), l
    for members in ([0, 1, 2], [0, 3], [3, 5], [0, 1, 2, 3, 4, 5], [2], [4]):
        g = M.GroupRef([cols[c] for c in members])
        for l in range(nv + 1):
            rows = np.concatenate([levels[c][l] for c in members], axis=1)
            assert g.distinct_tuples(l) == _brute_distinct(rows), (members, l)
    assert M.GroupRef([cols[0]]).counts[:3] == [12, 6, 3]


def test_every_way_of_factorising_gives_numpys_unique(monkeypatch):
    """_factorize: the table, the sample (complete, completed, given up) and the plain sort all return np.unique's result."""
    rng = np.random.default_rng(5)
    n = 1 << 18
    cases = {
        "few": rng.integers(0, 50, n) * 1000003,
        "runs": np.repeat(rng.integers(0, 1 << 40, n // 500), 500),
        "runs + strays": np.repeat(rng.integers(0, 1 << 40, n // 500), 500),
        "all distinct": rng.permutation(n).astype(np.int64) * 3,
        "half distinct": np.where(np.arange(n) % 2 == 0, 5, np.arange(n)),
    }
    cases["runs + strays"][rng.integers(0, n, 300)] = rng.integers(0, 1 << 40, 300)
    for lut in (1 << 22, 0):
        monkeypatch.setattr(M, "_LUT_SPACE", lut)
        for name, keys in cases.items():
            keys = keys.astype(np.int64)
            uniq, ids = M._factorize(keys, int(keys.max()) + 1)
            u, inv = np.unique(keys, return_inverse=True)
            assert np.array_equal(uniq, u) and np.array_equal(ids, inv.reshape(-1)), (lut, name)


# ---------------------------------------------------------------- the leader rule
def _run_tile_nodes_literal(npad, l):
    """kernels.hpp run_tile_nodes, line by line"""
    RUN_SEG, RUN_STAGE_LEVELS = 4096, 6
    if l == 0:
        return RUN_SEG
    s = (l - 1) // RUN_STAGE_LEVELS            # stage that emits level l
    n_in = npad >> (s * RUN_STAGE_LEVELS)      # nodes per column of the stage's input level
    seg = n_in if n_in < RUN_SEG else RUN_SEG
    return seg >> (l - s * RUN_STAGE_LEVELS)


def test_run_tile_nodes_is_the_kernels_rule():
    for nv in range(15, 27):
        for l in range(M._list_levels(nv)):
            assert M._run_tile_nodes(1 << nv, l) == _run_tile_nodes_literal(1 << nv, l), (nv, l)
            assert (1 << nv >> l) % M._run_tile_nodes(1 << nv, l) == 0
    # runs stage 2 (levels 13 ..) reads level 12 in segments of 4096 nodes: one segment per column up to 2^24 leaves, two at
    # 2^25, four at 2^26 -- only there are the tiles of these levels smaller than the level
    for nv, tiles in ((21, 1), (23, 1), (24, 1), (25, 2), (26, 4)):
        for l in range(13, M._list_levels(nv)):
            assert (1 << nv >> l) // M._run_tile_nodes(1 << nv, l) == tiles, (nv, l)
    for nv in (25, 26):  # ... while the levels below have had many tiles all along
        assert (1 << nv >> 12) // M._run_tile_nodes(1 << nv, 12) == (1 << nv) >> 18


def test_run_aware_model_counts_by_hand():
    """a constant column costs one hash per tile; a single change costs at most two more nodes per level"""
    nv = 16
    N = 1 << nv
    levels = M._list_levels(nv)
    tiles = sum((N >> l) // M._run_tile_nodes(N, l) for l in range(levels))
    const = np.full(N, 3, dtype=np.uint64)
    assert M._run_aware_hashed([const], levels) == tiles
    one = const.copy()
    one[12345:] = 4
    assert tiles < M._run_aware_hashed([one], levels) <= tiles + 1 + 2 * (levels - 1)
    assert M._run_aware_hashed([np.arange(N)], levels) == sum(N >> l for l in range(levels))  # nothing to copy


def test_one_leaf_in_the_last_stage2_segment_of_2p25_changes_everything_checked():
    """A 2^25 column of a few runs (two stage-2 segments of 2^24 leaves per column): one changed leaf in the LAST segment changes
    the reference root, the opening of its neighbour and the number of nodes the run-aware build must hash -- what the GPU
    tests compare is sensitive to every leaf, at the size where the tiles of the levels 13 .. first differ from the level."""
    nv = 25
    N = 1 << nv
    col = np.repeat(np.array([5, 9, 9, 2, 7, 7, 7, 1], dtype=np.uint64), N // 8)
    where = (1 << 24) + (1 << 23) + 12345          # inside the second stage-2 segment
    other = col.copy()
    other[where] += 1
    a, b = M.MerkleRef(col), M.MerkleRef(other)
    assert a.root != b.root
    assert a.hashes < 200 and b.hashes < 200 + 3 * nv
    sa, sb = a.open(where ^ 1), b.open(where ^ 1)
    assert sa[0][:32] != sb[0][:32] and sa[0][32:] == sb[0][32:] and sa[1:] == sb[1:]  # only the leaf-level sibling differs
    far_a, far_b = a.open(3), b.open(3)
    assert far_a[0][:32 * (nv - 1)] == far_b[0][:32 * (nv - 1)] and far_a[0][32 * (nv - 1):] != far_b[0][32 * (nv - 1):]
    levels = M._list_levels(nv)
    ha, hb = M._run_aware_hashed([col], levels), M._run_aware_hashed([other], levels)
    assert ha < hb <= ha + 2 + 2 * (levels - 1)
    for l in range(13, levels):  # the levels only the riding stage 2 produces count it too
        assert b.distinct(l) > a.distinct(l)
