#pragma once
// The host side of batched Merkle verification (api_merkle_verify.cpp, merkle_verify.hip), pure host code with no HIP in it so
// that it can be exercised without a GPU (tests/c_driver/verify_plan.cpp): the stable counting sort of the openings by height,
// the split of the sorted openings into chunks of bounded staging size, and the staging of one chunk -- each bucket's siblings
// and directions level-major, so that the lanes of a wave read one level of their openings from contiguous memory.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace zk {
namespace mv {

constexpr unsigned MAX_HEIGHT = 64;  // no tree over a 64-bit index is higher
constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// openings sorted by height: order[j] is the caller's index at sorted position j, soff[j] that opening's offset in the caller's
// packed siblings / directions (sum of the heights before it in the caller's order); bucket h holds [start[h], start[h + 1]).
// Stable: within a bucket the caller's order is kept.
struct Sorted {
    std::vector<uint32_t> order, soff;
    size_t start[MAX_HEIGHT + 2];
};
inline void sort_by_height(const size_t *heights, size_t k, Sorted &s) {
    size_t cnt[MAX_HEIGHT + 1] = {};
    for (size_t i = 0; i < k; i++) cnt[heights[i]]++;
    s.start[0] = 0;
    for (unsigned h = 0; h <= MAX_HEIGHT; h++) s.start[h + 1] = s.start[h] + cnt[h];
    size_t next[MAX_HEIGHT + 1];
    std::copy(s.start, s.start + MAX_HEIGHT + 1, next);
    s.order.resize(k);
    s.soff.resize(k);
    uint64_t off = 0;
    for (size_t i = 0; i < k; i++) {
        const size_t j = next[heights[i]]++;
        s.order[j] = (uint32_t)i;
        s.soff[j] = (uint32_t)off;
        off += heights[i];
    }
}

// a run of one bucket inside a chunk: sorted positions [base, base + cnt), all of one height; its siblings start at 32-byte
// slot sib (its directions at byte sib) of the chunk's sibling (direction) block
struct Piece {
    uint64_t base;
    uint32_t cnt, height;
    uint64_t sib;
};
// sorted positions [lo, hi) staged together: order u32 | roots 32 B | values u64 | siblings | directions, each block 256-byte
// aligned, at the offsets below from the chunk's staging base
struct Chunk {
    uint64_t lo, hi, sum_h;
    std::vector<Piece> pieces;
    size_t off_roots, off_vals, off_sib, off_dirs, bytes;
};
inline size_t staged_bytes(unsigned h) { return 4 + 32 + 8 + 33 * (size_t)h; }  // one opening, before alignment
inline void chunk_layout(Chunk &c) {
    const size_t n = c.hi - c.lo;
    c.off_roots = align256(4 * n);
    c.off_vals = c.off_roots + align256(32 * n);
    c.off_sib = c.off_vals + align256(8 * n);
    c.off_dirs = c.off_sib + align256(32 * c.sum_h);
    c.bytes = c.off_dirs + align256(c.sum_h);
}
// Splits the sorted openings into chunks whose staging fits max_bytes (a single opening always fits: 6 * 256 + 44 + 33 * 64
// bytes is the most one opening can need; max_bytes must be at least that).
inline std::vector<Chunk> plan_chunks(const Sorted &s, size_t k, size_t max_bytes) {
    std::vector<Chunk> out;
    size_t j = 0;
    while (j < k) {
        Chunk c{};
        c.lo = j;
        size_t raw = 0;
        while (j < k) {
            unsigned h = 0;
            while (s.start[h + 1] <= j) h++;  // (<= 65 steps; the bucket of position j)
            const size_t end = s.start[h + 1];
            // as many openings of this bucket as fit (5 * 256: the alignment of the five blocks)
            const size_t per = staged_bytes(h), room = max_bytes > raw + 5 * 256 ? max_bytes - raw - 5 * 256 : 0;
            const size_t take = std::min(end - j, room / per);
            if (take == 0) break;
            c.pieces.push_back(Piece{j, (uint32_t)take, h, c.sum_h});
            c.sum_h += (uint64_t)take * h;
            raw += take * per;
            j += take;
        }
        c.hi = j;
        chunk_layout(c);
        out.push_back(std::move(c));
    }
    return out;
}

// Fills the staging of chunk c at dst from the caller's arrays (roots 32 B, values u64, siblings 32 B and directions packed
// opening by opening).  Large chunks are split over up to `threads` threads.
inline void stage_chunk(const Sorted &s, const Chunk &c, const uint8_t *roots, const uint64_t *vals, const uint8_t *sib,
                        const uint8_t *dirs, uint8_t *dst, unsigned threads) {
    uint32_t *d_order = (uint32_t *)dst;
    uint8_t *d_roots = dst + c.off_roots, *d_sib = dst + c.off_sib, *d_dirs = dst + c.off_dirs;
    uint64_t *d_vals = (uint64_t *)(dst + c.off_vals);
    constexpr uint32_t SPAN = 4096;  // openings per work item
    struct Item {
        size_t piece;
        uint32_t lo, hi;  // lanes of the piece
    };
    std::vector<Item> items;
    for (size_t p = 0; p < c.pieces.size(); p++)
        for (uint32_t lo = 0; lo < c.pieces[p].cnt; lo += SPAN) items.push_back(Item{p, lo, std::min(c.pieces[p].cnt, lo + SPAN)});
    auto run = [&](const Item &it) {
        const Piece &p = c.pieces[it.piece];
        const size_t h = p.height;
        for (uint32_t i = it.lo; i < it.hi; i++) {
            const size_t j = p.base + i, n = j - c.lo;
            const uint32_t orig = s.order[j];
            d_order[n] = orig;
            memcpy(d_roots + 32 * n, roots + 32 * (size_t)orig, 32);
            d_vals[n] = vals[orig];
            const uint8_t *ss = sib + 32 * (size_t)s.soff[j], *sd = dirs + s.soff[j];
            for (size_t l = 0; l < h; l++) {
                memcpy(d_sib + 32 * (p.sib + l * p.cnt + i), ss + 32 * l, 32);
                d_dirs[p.sib + l * p.cnt + i] = sd[l];
            }
        }
    };
    unsigned nt = (unsigned)std::min<size_t>(threads, items.size());
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt <= 1 || c.bytes < ((size_t)1 << 20)) {
        for (const Item &it : items) run(it);
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t x; (x = next.fetch_add(1)) < items.size();) run(items[x]);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

}  // namespace mv
}  // namespace zk
