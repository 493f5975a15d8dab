// C ABI of libzigz_hip.so, part 6: batched Merkle commitments -- k independent SimpleMerkleTree builds, openings and
// CommitmentScheme openings in shared launches (merkle_batch.hip).
//
// One call to zigz_merkle_commit costs two allocations, an upload with its own round trip, a leaf launch and one launch per
// level, and another round trip for the root; a 2^10-leaf tree is ~2 K permutations, well under a microsecond of the chip, so
// a caller committing many small tables pays almost only for that.  Here a batch makes one device allocation (descriptors,
// values, trees and the eval words of all k tables), one upload, ceil(max height / 9) build launches and one launch that
// publishes the roots into pinned memory; an opening is one copy of descriptors, (the two launches of the batched MLE
// evaluation, mle_batch.hip,) one path launch and one hand-off.  Every tree is the dense tree of the single call, node for
// node, so roots and paths are byte-identical to it.
#include "api_internal.hpp"

#include <algorithm>

using namespace zk;

struct zigz_merkle_batch {
    zigz_ctx *ctx;
    size_t k;
    std::vector<uint64_t> n, npad;
    std::vector<unsigned> height;
    std::vector<size_t> vals_off;  // u32 words into d_vals (every table 16-byte aligned)
    std::vector<size_t> tree_off;  // nodes into d_tree (2 npad per tree)
    std::vector<size_t> sib_off;   // sum of the heights before the tree
    size_t sum_h;
    uint64_t max_n;                // the largest table
    size_t eval_wgs;               // workgroups of the opening's eval launch: sum of ceil(n / MLE_BATCH_CHUNK)
    void *d_mem;                   // the one allocation: descriptors | values | eval words | trees
    uint8_t *d_desc;
    size_t desc_bytes;
    uint32_t *d_vals;
    unsigned long long *d_eval;    // k results, then eval_wgs partial sums: an opening's launches write all of them, none is ever zeroed
    uint8_t *d_tree;
};

namespace {

constexpr size_t MAX_VALUES = (size_t)1 << 40;  // merkle_tree.zig:287 (the single call's device-size cap)

unsigned stages_of(unsigned h) { return h <= MB_STAGE_LEVELS ? 1 : (h + MB_STAGE_LEVELS - 1) / MB_STAGE_LEVELS; }
size_t open_desc_bytes(size_t k, size_t sum_h) {
    return align256(k * sizeof(MPathTab)) + align256(k * sizeof(MleBatchTab)) + 2 * sum_h * sizeof(uint32_t);
}

// Narrows the host tables into the packed u32 staging (table i at word vals_off[i]) and finds the first table holding a
// value >= p among the first `count` (count: none).  Large batches are split into chunks over up to 8 threads.
size_t narrow_tables(const uint64_t *const *values, const size_t *ns, size_t count, const std::vector<size_t> &off, uint32_t *dst) {
    constexpr size_t CHUNK = (size_t)1 << 18;
    struct Piece {
        size_t t, lo, hi;
    };
    std::vector<Piece> pieces;
    size_t total = 0;
    for (size_t i = 0; i < count; i++) {
        for (size_t lo = 0; lo < ns[i]; lo += CHUNK) pieces.push_back(Piece{i, lo, std::min(ns[i], lo + CHUNK)});
        total += ns[i];
    }
    std::vector<uint8_t> bad(pieces.size(), 0);
    auto run = [&](size_t j) {
        const Piece &p = pieces[j];
        const uint64_t *src = values[p.t];
        uint32_t *d = dst + off[p.t];
        uint64_t any = 0;
        for (size_t x = p.lo; x < p.hi; x++) {
            const uint64_t v = src[x];
            any |= (uint64_t)(v >= P);
            d[x] = (uint32_t)v;
        }
        bad[j] = (uint8_t)any;
    };
    unsigned nt = (unsigned)std::min<size_t>(8, total / (1 << 20));
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt <= 1) {
        for (size_t j = 0; j < pieces.size(); j++) run(j);
    } else {
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (size_t j; (j = next.fetch_add(1)) < pieces.size();) run(j);
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
    }
    for (size_t j = 0; j < pieces.size(); j++)
        if (bad[j]) return pieces[j].t;
    return count;
}

// the single call's checks of table i before its upload (zigz_merkle_commit)
zigz_status table_pre(size_t n, const void *p, bool dev) {
    if (n == 0) return ZIGZ_ERR_EMPTY_VALUES;              // merkle_tree.zig:284
    if (n > MAX_VALUES) return ZIGZ_ERR_TOO_MANY_VALUES;   // merkle_tree.zig:287
    if (!p || (dev && ((uintptr_t)p & 3))) return ZIGZ_ERR_INVALID_ARGUMENT;
    return ZIGZ_OK;
}

void batch_free(zigz_ctx *ctx, zigz_merkle_batch *b) {
    if (!b) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    if (b->d_mem) (void)hipFree(b->d_mem);
    delete b;
}

// Builds the k trees.  Exactly one of d_values (device tables) and values (host tables) is given; the host tables are narrowed
// into pinned memory and checked (< p) before anything is allocated on the device or launched.
zigz_status commit_run(zigz_ctx *ctx, const uint32_t *const *d_values, const uint64_t *const *values, const size_t *ns, size_t k,
                       uint8_t *roots, size_t *heights, zigz_merkle_batch **out, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    zigz_merkle_batch *b = new zigz_merkle_batch();
    b->ctx = ctx;
    b->k = k;
    b->n.assign(ns, ns + k);
    b->npad.resize(k);
    b->height.resize(k);
    b->vals_off = packed_offsets(ns, k);
    b->tree_off.resize(k);
    b->sib_off.resize(k);
    size_t nodes = 0, sum_h = 0, eval_wgs = 0;
    const size_t vw = b->vals_off[k];
    unsigned max_stages = 1;
    for (size_t i = 0; i < k; i++) {
        b->npad[i] = ceil_pow2(ns[i]);
        b->height[i] = log2_floor(b->npad[i]);
        b->tree_off[i] = nodes;
        nodes += 2 * b->npad[i];
        b->sib_off[i] = sum_h;
        sum_h += b->height[i];
        eval_wgs += (ns[i] + MLE_BATCH_CHUNK - 1) / MLE_BATCH_CHUNK;
        max_stages = std::max(max_stages, stages_of(b->height[i]));
    }
    b->sum_h = sum_h;
    b->eval_wgs = eval_wgs;
    b->max_n = *std::max_element(ns, ns + k);
    // the descriptors of every stage, one block: stage s serves the trees that reach level 9 s + 1
    std::vector<MBatchTab> tabs;
    std::vector<size_t> st_first(max_stages + 1), st_wgs(max_stages);
    for (unsigned s = 0; s < max_stages; s++) {
        st_first[s] = tabs.size();
        size_t wg = 0;
        for (size_t i = 0; i < k; i++) {
            if (s >= stages_of(b->height[i])) continue;
            const size_t n_in = b->npad[i] >> (s * MB_STAGE_LEVELS);
            MBatchTab t{};
            t.n = ns[i];
            t.npad = b->npad[i];
            t.lin = s * MB_STAGE_LEVELS;
            t.height = b->height[i];
            t.first_wg = (uint32_t)wg;
            t.idx = (uint32_t)i;
            tabs.push_back(t);
            wg += (n_in + MB_BLOCK - 1) / MB_BLOCK;
        }
        if (wg >= ((size_t)1 << 31)) {
            delete b;
            return ZIGZ_ERR_TOO_MANY_VALUES;
        }
        st_wgs[s] = wg;
    }
    st_first[max_stages] = tabs.size();
    b->desc_bytes = align256(std::max(tabs.size() * sizeof(MBatchTab), open_desc_bytes(k, sum_h)));
    const size_t vals_bytes = align256(vw * 4 + 16), eval_bytes = align256((k + eval_wgs) * 8);
    // pinned: roots | descriptors | (host form) values -- the last two go up in ONE copy, mirroring the device layout
    const size_t roots_bytes = align256(k * 32);
    const size_t up_bytes = b->desc_bytes + (values ? vw * 4 : 0);
    uint8_t *pin;
    zigz_status st = pinned(ctx, roots_bytes + up_bytes, &pin);
    if (st != ZIGZ_OK) {
        delete b;
        return st;
    }
    uint8_t *h_roots = pin, *h_up = pin + roots_bytes;
    if (values) {
        const size_t bad = narrow_tables(values, ns, k, b->vals_off, (uint32_t *)(h_up + b->desc_bytes));
        if (bad < k) {
            delete b;
            set_err(ctx, "table %zu contains a value >= p (not a canonical BabyBear element)", bad);
            return fail_at(bad_index, bad, ZIGZ_ERR_NOT_CANONICAL);
        }
    }
    if (hipMalloc(&b->d_mem, b->desc_bytes + vals_bytes + eval_bytes + nodes * 32) != hipSuccess) {
        (void)hipGetLastError();
        set_err(ctx, "hipMalloc of %zu bytes for a batch of %zu trees failed", b->desc_bytes + vals_bytes + eval_bytes + nodes * 32, k);
        delete b;
        return ZIGZ_ERR_OUT_OF_MEMORY;
    }
    b->d_desc = (uint8_t *)b->d_mem;
    b->d_vals = (uint32_t *)(b->d_desc + b->desc_bytes);
    b->d_eval = (unsigned long long *)((uint8_t *)b->d_vals + vals_bytes);
    b->d_tree = (uint8_t *)b->d_eval + eval_bytes;
    auto body = [&]() -> zigz_status {
        for (auto &t : tabs) {
            t.vals = b->d_vals + b->vals_off[t.idx];
            t.src = values ? t.vals : d_values[t.idx];
            t.tree = b->d_tree + b->tree_off[t.idx] * 32;
        }
        memcpy(h_up, tabs.data(), tabs.size() * sizeof(MBatchTab));
        HIPCHK(ctx, hipMemcpyAsync(b->d_desc, h_up, up_bytes, hipMemcpyHostToDevice, ctx->stream));
        const MBatchTab *d_tabs = (const MBatchTab *)b->d_desc;
        launch_mbatch_subtrees(d_tabs, (unsigned)(st_first[1] - st_first[0]), (unsigned)st_wgs[0], ctx->stream);
        for (unsigned s = 1; s < max_stages; s++)
            launch_mbatch_level(d_tabs + st_first[s], (unsigned)(st_first[s + 1] - st_first[s]), (unsigned)st_wgs[s], ctx->stream);
        const DoneFlag done = done_flag(ctx, 2);
        launch_mbatch_roots(d_tabs, (unsigned)k, h_roots, ctx->stream, done);  // stage 0 holds every tree, in order
        HIPCHK(ctx, hipGetLastError());
        CHK(wait_published(ctx, done));
        memcpy(roots, h_roots, k * 32);
        if (heights)
            for (size_t i = 0; i < k; i++) heights[i] = b->height[i];
        return ZIGZ_OK;
    };
    st = body();
    if (st != ZIGZ_OK || !out) {
        batch_free(ctx, b);
        return st;
    }
    *out = b;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// the openings of every tree at idx[i]; points != nullptr: CommitmentScheme.open (the evals first, into the handle's result words)
zigz_status open_run(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint64_t *idx, const uint64_t *points, uint64_t *values,
                     uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values) {
    const size_t k = b->k, sum_h = b->sum_h;
    // pinned: siblings | dirs | leaves | values (written by the path launch) | descriptors + factors (one copy up)
    const size_t sib_b = align256(sum_h * 32), dir_b = align256(sum_h), leaf_b = align256(k * 8), val_b = align256(k * 8);
    const size_t out_bytes = sib_b + dir_b + leaf_b + val_b, up_bytes = open_desc_bytes(k, sum_h);
    uint8_t *pin;
    CHK(pinned(ctx, out_bytes + up_bytes, &pin));
    MPathOut o;
    o.sib = pin;
    o.dirs = pin + sib_b;
    o.leaf = (uint64_t *)(pin + sib_b + dir_b);
    o.value = (uint64_t *)(pin + sib_b + dir_b + leaf_b);
    uint8_t *h_up = pin + out_bytes;
    MPathTab *hp = (MPathTab *)h_up;
    const size_t e_off = align256(k * sizeof(MPathTab)), f_off = e_off + align256(k * sizeof(MleBatchTab));
    std::vector<const uint32_t *> tables(k);
    for (size_t i = 0; i < k; i++) {
        MPathTab &p = hp[i];
        p.vals = tables[i] = b->d_vals + b->vals_off[i];  // the handle's copy: 16-byte aligned whatever the caller's table was
        p.tree = b->d_tree + b->tree_off[i] * 32;
        p.acc = points ? (const uint64_t *)(b->d_eval + i) : nullptr;
        p.npad = b->npad[i];
        p.index = idx[i];
        p.sib_off = b->sib_off[i];
        p.height = b->height[i];
        p.idx = (uint32_t)i;
    }
    if (points) mle_batch_fill(tables.data(), b->n.data(), k, points, false, (MleBatchTab *)(h_up + e_off), (uint32_t *)(h_up + f_off));
    HIPCHK(ctx, hipMemcpyAsync(b->d_desc, h_up, points ? up_bytes : k * sizeof(MPathTab), hipMemcpyHostToDevice, ctx->stream));
    if (points) {  // partial sums per workgroup, then table i's reduced result into d_eval[i]: device words, so nothing to signal
        const MleBatchTab *d_tabs = (const MleBatchTab *)(b->d_desc + e_off);
        launch_mle_batch_eval(d_tabs, (unsigned)k, (unsigned)b->eval_wgs, (const uint32_t *)(b->d_desc + f_off), b->d_eval + k, ctx->stream);
        launch_mle_batch_finish(d_tabs, (unsigned)k, b->d_eval + k, (uint64_t *)b->d_eval, ctx->stream, DoneFlag());
    }
    const DoneFlag done = done_flag(ctx, 2);
    launch_mbatch_paths((const MPathTab *)b->d_desc, (unsigned)k, o, ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    if (sum_h) {
        memcpy(siblings, o.sib, sum_h * 32);
        memcpy(dirs, o.dirs, sum_h);
    }
    memcpy(leaf_values, o.leaf, k * 8);
    if (points) memcpy(values, o.value, k * 8);
    return ZIGZ_OK;
}

}  // namespace

extern "C" zigz_status zigz_dev_merkle_commit_batch(zigz_ctx *ctx, const uint32_t *const *d_values, const size_t *ns, size_t k,
                                                    uint8_t *roots, size_t *heights, zigz_merkle_batch **out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !d_values || !ns || !roots) return ZIGZ_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < k; i++) {
        const zigz_status st = table_pre(ns[i], d_values[i], true);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
    }
    return commit_run(ctx, d_values, nullptr, ns, k, roots, heights, out, bad_index);
}

extern "C" zigz_status zigz_merkle_commit_batch(zigz_ctx *ctx, const uint64_t *const *values, const size_t *ns, size_t k,
                                                uint8_t *roots, size_t *heights, zigz_merkle_batch **out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !values || !ns || !roots) return ZIGZ_ERR_INVALID_ARGUMENT;
    ZIGZ_NOTHROW_BEGIN
    CHK(checks_in_call_order(values, ns, k, bad_index, [&](size_t *f) -> zigz_status {
        for (size_t i = 0; i < k; i++) {
            const zigz_status st = table_pre(ns[i], values[i], false);
            if (st != ZIGZ_OK) return fail_at(f, i, st);
        }
        return ZIGZ_OK;
    }));
    return commit_run(ctx, nullptr, values, ns, k, roots, heights, out, bad_index);  // (checks the values while it narrows them)
    ZIGZ_NOTHROW_END(ctx)
}

extern "C" zigz_status zigz_merkle_open_batch(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint64_t *indices, uint8_t *siblings,
                                              uint8_t *dirs, uint64_t *leaf_values, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !b || b->ctx != ctx || !indices || !leaf_values || (b->sum_h && (!siblings || !dirs))) return ZIGZ_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < b->k; i++)
        if (indices[i] >= b->n[i]) return fail_at(bad_index, i, ZIGZ_ERR_INDEX_OUT_OF_BOUNDS);  // merkle_tree.zig:325
    ZIGZ_NOTHROW_BEGIN
    return open_run(ctx, b, indices, nullptr, nullptr, siblings, dirs, leaf_values);
    ZIGZ_NOTHROW_END(ctx)
}

extern "C" zigz_status zigz_commit_open_batch(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint64_t *points, uint64_t *values,
                                              uint64_t *indices, uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values,
                                              size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !b || b->ctx != ctx || !values || !indices || !leaf_values || (b->sum_h && (!points || !siblings || !dirs)))
        return ZIGZ_ERR_INVALID_ARGUMENT;
    // k_mle_batch_eval sums exactly up to 2^MLE_BATCH_MAX_LOG2_N values per table in at most MLE_BATCH_MAX_WGS chunks.  A table
    // of 2^33 values needs 32 GiB of values and 512 GiB of tree, 2^24 chunks are 2^37 values: no handle that large fits the device.
    if (b->eval_wgs > MLE_BATCH_MAX_WGS || b->max_n > ((uint64_t)1 << MLE_BATCH_MAX_LOG2_N)) return ZIGZ_ERR_INVALID_ARGUMENT;
    ZIGZ_NOTHROW_BEGIN
    std::vector<uint64_t> idx(b->k);
    for (size_t i = 0; i < b->k; i++) {
        const zigz_status st = mle_check(b->n[i]);  // polynomial_commit.zig:86 (Multilinear.init)
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        const unsigned nv = b->height[i];
        const uint64_t *pt = points + b->sib_off[i];
        for (unsigned v = 0; v < nv; v++)
            if (pt[v] >= P) return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        idx[i] = nv == 0 ? 0 : pt[0] % ((uint64_t)1 << nv);  // pointToIndex, :178-183
    }
    CHK(open_run(ctx, b, idx.data(), points, values, siblings, dirs, leaf_values));
    memcpy(indices, idx.data(), b->k * 8);
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// ---- many openings per tree (merkle_batch.hip: k_mbatch_open_many)
namespace {

// the descriptors of openings [c.lo, c.hi) into hd
void fill_descs(const mo::Chunk &c, const uint32_t *trees, const uint64_t *indices, const std::vector<uint64_t> &off, mo::Desc *hd) {
    for (size_t j = c.lo; j < c.hi; j++) hd[j - c.lo] = mo::Desc{indices[j], trees[j], (uint32_t)(off[j] - c.slot0)};
}
void fill_trees(const zigz_merkle_batch *b, MOpenTree *ht) {
    for (size_t i = 0; i < b->k; i++)
        ht[i] = MOpenTree{b->d_tree + b->tree_off[i] * 32, b->d_vals + b->vals_off[i], b->npad[i], b->height[i], 0};
}

// Host form: every chunk's siblings, directions, leaves and roots are written by the kernel into one half of a pinned region
// and copied to the caller while the next chunk runs.  A half: tree table (chunk 0 only) | descriptors | outputs.
zigz_status open_many_host(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint32_t *trees, const uint64_t *indices,
                           const std::vector<uint64_t> &off, size_t k, uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values,
                           uint8_t *roots) {
    const std::vector<mo::Chunk> chunks = mo::plan_chunks(off, k, OPEN_CHUNK_BYTES, roots != nullptr);
    const size_t tabs_bytes = align256(b->k * sizeof(MOpenTree));
    size_t most = 0, most_n = 0;
    for (const mo::Chunk &c : chunks) {
        most = std::max(most, c.bytes);
        most_n = std::max(most_n, c.hi - c.lo);
    }
    const size_t half_bytes = tabs_bytes + most;
    uint8_t *pin;
    CHK(pinned(ctx, (chunks.size() > 1 ? 2 : 1) * half_bytes, &pin));
    void *ws;
    CHK(ws_get(ctx, WS_OPEN, tabs_bytes + most_n * sizeof(mo::Desc), &ws));
    const MOpenTree *d_trees = (const MOpenTree *)ws;
    mo::Desc *d_desc = (mo::Desc *)((uint8_t *)ws + tabs_bytes);
    auto launch = [&](size_t ci, DoneFlag *done) -> zigz_status {
        const mo::Chunk &c = chunks[ci];
        uint8_t *h = pin + (ci & 1) * half_bytes, *st = h + tabs_bytes;
        const size_t n = c.hi - c.lo;
        fill_descs(c, trees, indices, off, (mo::Desc *)st);
        if (ci == 0) {  // the tree table rides in front of the first chunk's descriptors: one copy per chunk
            fill_trees(b, (MOpenTree *)h);
            HIPCHK(ctx, hipMemcpyAsync(ws, h, tabs_bytes + n * sizeof(mo::Desc), hipMemcpyHostToDevice, ctx->stream));
        } else {  // (the previous chunk's launch reads d_desc: the copy queues behind it on the stream)
            HIPCHK(ctx, hipMemcpyAsync(d_desc, st, n * sizeof(mo::Desc), hipMemcpyHostToDevice, ctx->stream));
        }
        const MOpenOut o{st + c.off_sib, st + c.off_dirs, (uint64_t *)(st + c.off_leaf), roots ? st + c.off_roots : nullptr};
        *done = done_flag(ctx, 3 + (int)(ci & 1));
        launch_mbatch_open_many(d_trees, d_desc, (unsigned)n, (unsigned)c.slots, c.zero_height, o, false, ctx->stream, *done);
        HIPCHK(ctx, hipGetLastError());
        return ZIGZ_OK;
    };
    auto take = [&](size_t ci) {
        const mo::Chunk &c = chunks[ci];
        const uint8_t *st = pin + (ci & 1) * half_bytes + tabs_bytes;
        const size_t n = c.hi - c.lo;
        if (c.slots) {
            memcpy(siblings + 32 * c.slot0, st + c.off_sib, 32 * c.slots);
            memcpy(dirs + c.slot0, st + c.off_dirs, c.slots);
        }
        memcpy(leaf_values + c.lo, st + c.off_leaf, 8 * n);
        if (roots) memcpy(roots + 32 * c.lo, st + c.off_roots, 32 * n);
    };
    return run_open_chunks(ctx, chunks.size(), launch, take);
}

// Device form: one launch writes the caller's device arrays; only the tree table and the descriptors go up, from a pinned
// region of their own that the next call does not touch before this call's upload has left it.
zigz_status open_many_dev(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint32_t *trees, const uint64_t *indices,
                          const std::vector<uint64_t> &off, size_t k, uint8_t *d_siblings, uint8_t *d_dirs, uint64_t *d_leaf_values,
                          uint8_t *d_roots) {
    const size_t tabs_bytes = align256(b->k * sizeof(MOpenTree)), up_bytes = tabs_bytes + k * sizeof(mo::Desc);
    uint8_t *h_up;
    CHK(upload_region(ctx, up_bytes, &h_up));
    void *ws;
    CHK(ws_get(ctx, WS_OPEN, up_bytes, &ws));
    mo::Chunk c{};
    c.hi = k;
    bool zero_height = false;
    for (size_t j = 0; j < k && !zero_height; j++) zero_height = off[j + 1] == off[j];
    fill_trees(b, (MOpenTree *)h_up);
    fill_descs(c, trees, indices, off, (mo::Desc *)(h_up + tabs_bytes));
    HIPCHK(ctx, hipMemcpyAsync(ws, h_up, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_open, ctx->stream));
    const MOpenOut o{d_siblings, d_dirs, d_leaf_values, d_roots};
    launch_mbatch_open_many((const MOpenTree *)ws, (const mo::Desc *)((uint8_t *)ws + tabs_bytes), (unsigned)k, (unsigned)off[k],
                            zero_height, o, true, ctx->stream, DoneFlag());
    HIPCHK(ctx, hipGetLastError());
    return ZIGZ_OK;
}

zigz_status open_many(zigz_ctx *ctx, const zigz_merkle_batch *b, bool dev, size_t k, const uint32_t *trees, const uint64_t *indices,
                      uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values, uint8_t *roots, size_t *heights, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !b || b->ctx != ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (dev && (((uintptr_t)siblings | (uintptr_t)roots) & 15 || (uintptr_t)leaf_values & 7)) return ZIGZ_ERR_INVALID_ARGUMENT;
    size_t bad = 0;
    switch (mo::check_openings(k, trees, indices, b->k, b->n.data(), 0, &bad)) {
    case mo::OK: break;
    case mo::BAD_ARGUMENT: return ZIGZ_ERR_INVALID_ARGUMENT;
    case mo::BAD_TREE:
        set_err(ctx, "opening %zu names tree %u of a batch of %zu", bad, trees[bad], b->k);
        return fail_at(bad_index, bad, ZIGZ_ERR_INVALID_ARGUMENT);
    case mo::BAD_INDEX: return fail_at(bad_index, bad, ZIGZ_ERR_INDEX_OUT_OF_BOUNDS);  // merkle_tree.zig:325 (values.len)
    }
    ZIGZ_NOTHROW_BEGIN
    std::vector<uint64_t> off;
    mo::offsets(k, trees, b->height.data(), off);
    if (!leaf_values || (off[k] && (!siblings || !dirs))) return ZIGZ_ERR_INVALID_ARGUMENT;
    CHK(dev ? open_many_dev(ctx, b, trees, indices, off, k, siblings, dirs, leaf_values, roots)
            : open_many_host(ctx, b, trees, indices, off, k, siblings, dirs, leaf_values, roots));
    if (heights)
        for (size_t j = 0; j < k; j++) heights[j] = b->height[trees[j]];
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_merkle_open_many(zigz_ctx *ctx, const zigz_merkle_batch *b, size_t k, const uint32_t *trees,
                                             const uint64_t *indices, uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values,
                                             uint8_t *roots, size_t *heights, size_t *bad_index) {
    return open_many(ctx, b, false, k, trees, indices, siblings, dirs, leaf_values, roots, heights, bad_index);
}

extern "C" zigz_status zigz_dev_merkle_open_many(zigz_ctx *ctx, const zigz_merkle_batch *b, size_t k, const uint32_t *trees,
                                                 const uint64_t *indices, uint8_t *d_siblings, uint8_t *d_dirs,
                                                 uint64_t *d_leaf_values, uint8_t *d_roots, size_t *heights, size_t *bad_index) {
    return open_many(ctx, b, true, k, trees, indices, d_siblings, d_dirs, d_leaf_values, d_roots, heights, bad_index);
}

extern "C" void zigz_merkle_batch_destroy(zigz_ctx *ctx, zigz_merkle_batch *b) {
    ZIGZ_ENTER(ctx);
    batch_free(ctx ? ctx : (b ? b->ctx : nullptr), b);
}
