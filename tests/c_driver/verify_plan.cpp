// The host side of the batched Merkle verification (zigz_amd/csrc/verify_plan.hpp) without a GPU: the counting sort by height,
// the chunk plan and the level-major staging, on ragged height mixes, read back through the layout the kernel reads.
// Usage: verify_plan  -> prints "verify_plan: N case(s), 0 failure(s)"
#include <stdio.h>

#include <random>

#include "verify_plan.hpp"

using namespace zk::mv;

static int failures = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                  \
    } while (0)

static void run_case(const std::vector<size_t> &heights, size_t max_bytes, unsigned threads, uint64_t seed) {
    const size_t k = heights.size();
    std::vector<size_t> off(k + 1, 0);
    for (size_t i = 0; i < k; i++) off[i + 1] = off[i] + heights[i];
    std::mt19937_64 rng(seed);
    std::vector<uint8_t> roots(32 * k), sib(32 * off[k] + 1), dirs(off[k] + 1);
    std::vector<uint64_t> vals(k);
    for (auto &b : roots) b = (uint8_t)rng();
    for (auto &b : sib) b = (uint8_t)rng();
    for (auto &b : dirs) b = (uint8_t)rng();
    for (auto &v : vals) v = rng();

    Sorted s;
    sort_by_height(heights.data(), k, s);
    // a stable permutation, sorted by height, with the caller's sibling offsets
    std::vector<uint8_t> seen(k, 0);
    for (size_t j = 0; j < k; j++) {
        const uint32_t i = s.order[j];
        EXPECT(i < k && !seen[i]);
        if (i >= k) return;
        seen[i] = 1;
        EXPECT(s.soff[j] == off[i]);
        EXPECT(j >= s.start[heights[i]] && j < s.start[heights[i] + 1]);
        if (j > 0) {
            const uint32_t p = s.order[j - 1];
            EXPECT(heights[p] < heights[i] || (heights[p] == heights[i] && p < i));
        }
    }
    EXPECT(s.start[0] == 0 && s.start[MAX_HEIGHT + 1] == k);

    const std::vector<Chunk> chunks = plan_chunks(s, k, max_bytes);
    uint64_t next = 0;
    for (const Chunk &c : chunks) {
        EXPECT(c.lo == next && c.hi > c.lo && c.bytes <= max_bytes);
        next = c.hi;
        uint64_t pos = c.lo, slot = 0;
        for (const Piece &p : c.pieces) {  // contiguous runs of one height, siblings packed piece after piece
            EXPECT(p.base == pos && p.cnt > 0 && p.sib == slot);
            for (uint64_t j = p.base; j < p.base + p.cnt; j++) EXPECT(heights[s.order[j]] == p.height);
            pos += p.cnt;
            slot += (uint64_t)p.cnt * p.height;
        }
        EXPECT(pos == c.hi && slot == c.sum_h);
        std::vector<uint8_t> st(c.bytes, 0xEE);
        stage_chunk(s, c, roots.data(), vals.data(), sib.data(), dirs.data(), st.data(), threads);
        const uint32_t *order = (const uint32_t *)st.data();
        const uint64_t *sv = (const uint64_t *)(st.data() + c.off_vals);
        for (const Piece &p : c.pieces)
            for (uint32_t i = 0; i < p.cnt; i++) {  // what lane i of the piece reads
                const uint64_t n = p.base + i - c.lo;
                const uint32_t o = order[n];
                EXPECT(o == s.order[p.base + i]);
                EXPECT(memcmp(st.data() + c.off_roots + 32 * n, roots.data() + 32 * (size_t)o, 32) == 0);
                EXPECT(sv[n] == vals[o]);
                for (uint32_t l = 0; l < p.height; l++) {
                    EXPECT(memcmp(st.data() + c.off_sib + 32 * (p.sib + (uint64_t)l * p.cnt + i), sib.data() + 32 * (off[o] + l), 32) == 0);
                    EXPECT(st[c.off_dirs + p.sib + (uint64_t)l * p.cnt + i] == dirs[off[o] + l]);
                }
            }
    }
    EXPECT(next == k);
}

int main() {
    int cases = 0;
    std::mt19937_64 rng(7);
    const size_t budgets[] = {4096, 65536, (size_t)1 << 20, (size_t)32 << 20};
    for (int t = 0; t < 40; t++) {
        const size_t k = t < 5 ? (size_t)t : 1 + rng() % (t < 30 ? 3000 : 70000);
        std::vector<size_t> h(k);
        const int mix = t % 4;
        for (auto &x : h)
            x = mix == 0 ? rng() % 25                            // 0 .. 24
                : mix == 1 ? (rng() % 8 ? 20 : rng() % 65)       // mostly 20, a few of any height
                : mix == 2 ? 64 - rng() % 3                      // the highest paths
                           : (rng() % 2 ? 0 : 1 + rng() % 12);   // many empty paths
        run_case(h, budgets[t % 4], t % 2 ? 8 : 1, 1000 + t);
        cases++;
    }
    printf("verify_plan: %d case(s), %d failure(s)\n", cases, failures);
    return failures != 0;
}
