#pragma once
// The host side of the many-openings entries (zigz_merkle_open_many, zigz_dev_merkle_open_many, zigz_commit_open_many), pure
// host code with no HIP in it so that it can be exercised without a GPU (tests/c_driver/open_plan.cpp): the argument checks,
// the prefix of sibling offsets, and the split of a call into chunks whose staging fits a bounded piece of pinned memory.
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zk {
namespace mo {

constexpr size_t MAX_OPENINGS = (size_t)1 << 22;  // ZIGZ_VERIFY_BATCH_MAX: what one verify call takes
constexpr unsigned MAX_HEIGHT = 64;               // no tree over a 64-bit index is higher
constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// one launch serves a whole call of the device form: two 16-byte work items per sibling digest
static_assert(MAX_OPENINGS * MAX_HEIGHT * 2 < ((uint64_t)1 << 31), "the work items of one call fit one launch");

// what the device reads per opening (16 bytes)
struct Desc {
    uint64_t index;
    uint32_t tree;  // tree of the batch / column of the job
    uint32_t off;   // batch: first sibling slot of the opening within its chunk; job: the opening's position within its chunk
};
static_assert(sizeof(Desc) == 16, "descriptor layout");

enum Check { OK = 0, BAD_ARGUMENT, BAD_TREE, BAD_INDEX };
// The checks of a call's (tree, index) pairs, reading nothing when k is 0 or too large.  Tree t has ns[t] values (ns ==
// nullptr: every tree has n_all).  BAD_TREE / BAD_INDEX: *bad is the first offending j, whichever of the two it fails.
inline Check check_openings(size_t k, const uint32_t *trees, const uint64_t *indices, size_t n_trees, const uint64_t *ns,
                            uint64_t n_all, size_t *bad) {
    if (k == 0) return OK;
    if (k > MAX_OPENINGS || !trees || !indices) return BAD_ARGUMENT;
    for (size_t j = 0; j < k; j++) {
        if (trees[j] >= n_trees) {
            *bad = j;
            return BAD_TREE;
        }
        if (indices[j] >= (ns ? ns[trees[j]] : n_all)) {
            *bad = j;
            return BAD_INDEX;
        }
    }
    return OK;
}

// off[j] = sum of the heights of the openings before j (off[k]: all sibling slots of the call); heights[t]: height of tree t
inline void offsets(size_t k, const uint32_t *trees, const unsigned *heights, std::vector<uint64_t> &off) {
    off.resize(k + 1);
    uint64_t o = 0;
    for (size_t j = 0; j < k; j++) {
        off[j] = o;
        o += heights[trees[j]];
    }
    off[k] = o;
}

// Openings [lo, hi) of a call staged together, never a part of an opening: descriptors (up) | siblings 32 B | directions |
// leaf values u64 | roots 32 B (down), each block 256-byte aligned at the offsets below from the chunk's staging base.
struct Chunk {
    size_t lo, hi;
    uint64_t slot0, slots;  // its sibling slots: [slot0, slot0 + slots) of the call
    bool zero_height;       // holds an opening without siblings (served by the one-thread-per-opening pass)
    size_t off_sib, off_dirs, off_leaf, off_roots, bytes;
};
inline size_t staged_bytes(uint64_t h, bool roots) { return 16 + 33 * (size_t)h + 8 + (roots ? 32 : 0); }  // one opening, before alignment
// Splits openings with the offset prefix `off` into chunks whose staging fits max_bytes (at least 5 * 256 + 56 + 33 * 64, so
// that a single opening always fits).
inline std::vector<Chunk> plan_chunks(const std::vector<uint64_t> &off, size_t k, size_t max_bytes, bool roots) {
    std::vector<Chunk> out;
    size_t j = 0;
    while (j < k) {
        Chunk c{};
        c.lo = j;
        c.slot0 = off[j];
        size_t raw = 0;
        while (j < k) {
            const uint64_t h = off[j + 1] - off[j];
            const size_t need = staged_bytes(h, roots);
            if (j > c.lo && raw + need + 5 * 256 > max_bytes) break;
            raw += need;
            c.zero_height |= h == 0;
            j++;
        }
        c.hi = j;
        c.slots = off[j] - c.slot0;
        const size_t n = c.hi - c.lo;
        c.off_sib = align256(16 * n);
        c.off_dirs = c.off_sib + align256(32 * c.slots);
        c.off_leaf = c.off_dirs + align256(c.slots);
        c.off_roots = c.off_leaf + align256(8 * n);
        c.bytes = c.off_roots + (roots ? align256(32 * n) : 0);
        out.push_back(c);
    }
    return out;
}

}  // namespace mo
}  // namespace zk
