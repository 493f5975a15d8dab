// The host side of the many-openings entries (zigz_amd/csrc/open_plan.hpp) without a GPU: the argument checks, the prefix of
// sibling offsets over mixed heights (0 included) and the split of a call into chunks that never cut an opening.
// Usage: open_plan  -> prints "open_plan: N case(s), 0 failure(s)"
#include <stdio.h>

#include <random>

#include "open_plan.hpp"

using namespace zk::mo;

static int failures = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                  \
    } while (0)

// the tables of test_gpu_merkle_open_many: 1, 2, 3, 5, 8, 257, 4097 values
static const uint64_t NS[] = {1, 2, 3, 5, 8, 257, 4097};
static const unsigned HS[] = {0, 1, 2, 3, 3, 9, 13};
static const size_t NT = 7;

static void checks() {
    size_t bad = 99;
    const uint32_t t1[] = {6};
    const uint64_t i1[] = {0};
    // k == 0 and k == max + 1 read nothing (the arrays hold one entry / are null)
    EXPECT(check_openings(0, nullptr, nullptr, NT, NS, 0, &bad) == OK && bad == 99);
    EXPECT(check_openings(MAX_OPENINGS + 1, t1, i1, NT, NS, 0, &bad) == BAD_ARGUMENT && bad == 99);
    EXPECT(check_openings(1, nullptr, i1, NT, NS, 0, &bad) == BAD_ARGUMENT);
    EXPECT(check_openings(1, t1, nullptr, NT, NS, 0, &bad) == BAD_ARGUMENT && bad == 99);
    EXPECT(check_openings(1, t1, i1, NT, NS, 0, &bad) == OK && bad == 99);
    // the first offender of two, for a tree id and for an index; 4096 is the last valid index of the 4097-value table
    const uint32_t t2[] = {0, 6, 7, 3, 7};
    const uint64_t i2[] = {0, 4096, 0, 1, 0};
    EXPECT(check_openings(5, t2, i2, NT, NS, 0, &bad) == BAD_TREE && bad == 2);
    const uint32_t t3[] = {6, 6, 6, 0, 6};
    const uint64_t i3[] = {4096, 0, 4097, 0, 4097};
    bad = 99;
    EXPECT(check_openings(5, t3, i3, NT, NS, 0, &bad) == BAD_INDEX && bad == 2);
    // whichever comes first wins: an index out of range before a tree out of range, and the other way round
    const uint32_t t4[] = {1, 9};
    const uint64_t i4[] = {2, 0};
    EXPECT(check_openings(2, t4, i4, NT, NS, 0, &bad) == BAD_INDEX && bad == 0);
    const uint32_t t5[] = {9, 1};
    const uint64_t i5[] = {0, 2};
    EXPECT(check_openings(2, t5, i5, NT, NS, 0, &bad) == BAD_TREE && bad == 0);
    // trees of one size (a commit job's columns)
    const uint32_t t6[] = {42, 0, 43};
    const uint64_t i6[] = {1023, 1024, 0};
    EXPECT(check_openings(3, t6, i6, 43, nullptr, 1024, &bad) == BAD_INDEX && bad == 1);
    EXPECT(check_openings(1, t6, i6, 43, nullptr, 1024, &bad) == OK);
}

static void run_case(const std::vector<uint32_t> &trees, size_t max_bytes, bool roots) {
    const size_t k = trees.size();
    std::vector<uint64_t> off;
    offsets(k, trees.data(), HS, off);
    EXPECT(off.size() == k + 1 && off[0] == 0);
    for (size_t j = 0; j < k; j++) EXPECT(off[j + 1] - off[j] == HS[trees[j]]);
    const std::vector<Chunk> chunks = plan_chunks(off, k, max_bytes, roots);
    size_t next = 0;
    for (const Chunk &c : chunks) {
        const size_t n = c.hi - c.lo;
        // whole openings, in order, none left out: a chunk's slots are exactly those of its openings
        EXPECT(c.lo == next && c.hi > c.lo && c.hi <= k);
        EXPECT(c.slot0 == off[c.lo] && c.slots == off[c.hi] - off[c.lo]);
        EXPECT(c.bytes <= max_bytes || n == 1);
        bool zero = false;
        for (size_t j = c.lo; j < c.hi; j++) zero |= HS[trees[j]] == 0;
        EXPECT(zero == c.zero_height);
        // the blocks do not overlap and are aligned for the kernel's 16-byte stores
        EXPECT(c.off_sib >= 16 * n && c.off_sib % 256 == 0);
        EXPECT(c.off_dirs >= c.off_sib + 32 * c.slots && c.off_dirs % 256 == 0);
        EXPECT(c.off_leaf >= c.off_dirs + c.slots && c.off_leaf % 256 == 0);
        EXPECT(c.off_roots >= c.off_leaf + 8 * n && c.off_roots % 256 == 0);
        EXPECT(c.bytes >= c.off_roots + (roots ? 32 * n : 0));
        // a chunk is full: the next opening would not have fitted
        if (c.hi < k) {
            size_t raw = 0;
            for (size_t j = c.lo; j <= c.hi; j++) raw += staged_bytes(HS[trees[j]], roots);
            EXPECT(raw + 5 * 256 > max_bytes);
        }
        next = c.hi;
    }
    EXPECT(next == k);
    EXPECT(k != 0 || chunks.empty());
}

int main() {
    checks();
    int cases = 1;
    std::mt19937_64 rng(11);
    const size_t budgets[] = {4096, 65536, (size_t)1 << 20, (size_t)32 << 20};
    for (int t = 0; t < 40; t++) {
        const size_t k = t < 5 ? (size_t)t : 1 + rng() % (t < 30 ? 3000 : 200000);
        std::vector<uint32_t> trees(k);
        const int mix = t % 4;
        for (auto &x : trees)
            x = mix == 0 ? (uint32_t)(rng() % NT)                    // every height
                : mix == 1 ? (uint32_t)(rng() % 8 ? 6 : rng() % NT)  // mostly the highest
                : mix == 2 ? 0                                       // no siblings at all
                           : (uint32_t)(rng() % 2 ? 0 : 5);          // empty paths between long ones
        run_case(trees, budgets[t % 4], t % 3 != 0);
        cases++;
    }
    printf("open_plan: %d case(s), %d failure(s)\n", cases, failures);
    return failures != 0;
}
