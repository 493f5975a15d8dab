// C ABI of libzigz_hip.so, part 7: batched Merkle verification -- SimpleMerkleTree.verify for k independent openings in shared
// launches (merkle_verify.hip); CommitmentScheme.batchVerify is "no opening rejected".
//
// The host checks one opening with height + 1 sequential SHA3 calls, one opening after the other.  Here one lane takes one
// opening: the openings are sorted by height on the host (verify_plan.hpp), each bucket of one height owns whole workgroups,
// and a lane writes its verdict byte into pinned memory at the caller's index.  The rejects are counted on the device and
// published by one k_publish launch behind the last verify launch, whose completion word the host polls.
//
// Host form: the values, roots, siblings and directions are staged per chunk into one half of a pinned region (each bucket's
// siblings and directions level-major), on up to 8 threads, and go up in one copy per chunk; while the device verifies one
// chunk the host fills the other half.  A chunk holds at most VERIFY_CHUNK_BYTES of staging, so the pinned region stays
// bounded whatever k is.  Device form: only the sort (order and sibling offsets, 8 bytes per opening) goes up; the lanes
// gather from the caller's layout.
#include "api_internal.hpp"

#include "verify_plan.hpp"

using namespace zk;

namespace {

constexpr size_t VERIFY_CHUNK_BYTES = (size_t)32 << 20;  // staging per chunk (one half of the pinned region), DESIGN.md s7d
constexpr size_t TABS_BYTES = mv::align256((mv::MAX_HEIGHT + 1) * sizeof(MVerifyTab));  // the descriptors of one launch
constexpr unsigned PAUSE_MIN_WAVES = 4096;  // launches of at least this many waves hash with the re-arm pauses
static_assert(sizeof(MVerifyTab) == 40, "descriptor layout");

bool pause_for(const zigz_ctx *ctx, size_t nwg) {
    if (ctx->verify_pause) return ctx->verify_pause == 1;
    return nwg * (MV_TPB / 64) >= PAUSE_MIN_WAVES;
}

// the descriptors of one launch over `pieces` (host form: sib / dirs point into the chunk's device staging); returns the
// number of workgroups
template <class Pieces>
unsigned make_tabs(const Pieces &pieces, MVerifyTab *tabs, const uint8_t *d_sib, const uint8_t *d_dirs) {
    unsigned wg = 0, n = 0;
    for (const mv::Piece &p : pieces) {
        MVerifyTab &t = tabs[n++];
        t.sib = d_sib ? d_sib + 32 * p.sib : nullptr;
        t.dirs = d_dirs ? d_dirs + p.sib : nullptr;
        t.base = p.base;
        t.cnt = p.cnt;
        t.height = p.height;
        t.first_wg = wg;
        t.pad = 0;
        wg += (p.cnt + MV_TPB - 1) / MV_TPB;
    }
    return wg;
}

// Runs the verification of k openings (arguments checked).  Host form: roots / vals / sib / dirs are host arrays; device
// form (dev): device arrays.  Verdicts and the reject count come back through pinned memory.
zigz_status verify_run(zigz_ctx *ctx, bool dev, size_t k, const uint8_t *roots, const size_t *heights, const uint64_t *vals,
                       const uint8_t *sib, const uint8_t *dirs, uint8_t *verdicts, size_t *n_rejected) {
    ZIGZ_NOTHROW_BEGIN
    mv::Sorted s;
    mv::sort_by_height(heights, k, s);
    // pinned: reject count | verdicts (the caller's order) | staging (host form: two halves; device form: one upload)
    const size_t out_bytes = 256 + mv::align256(k);
    std::vector<mv::Chunk> chunks;
    size_t stage_bytes;
    if (dev) {
        stage_bytes = TABS_BYTES + mv::align256(4 * k) * 2;
    } else {
        chunks = mv::plan_chunks(s, k, VERIFY_CHUNK_BYTES);
        size_t most = 0;
        for (const mv::Chunk &c : chunks) most = std::max(most, c.bytes);
        stage_bytes = TABS_BYTES + most;
    }
    uint8_t *pin;
    CHK(pinned(ctx, out_bytes + (dev || chunks.size() == 1 ? 1 : 2) * stage_bytes, &pin));
    unsigned long long *h_rej = (unsigned long long *)pin;
    uint8_t *h_verd = pin + 256, *half[2] = {pin + out_bytes, pin + out_bytes + stage_bytes};
    // device: reject counter | staging of one launch
    void *ws;
    CHK(ws_get(ctx, WS_VERIFY, 256 + stage_bytes, &ws));
    unsigned long long *d_rej = (unsigned long long *)ws;
    uint8_t *d_stage = (uint8_t *)ws + 256;
    HIPCHK(ctx, hipMemsetAsync(d_rej, 0, 8, ctx->stream));
    MVerifyArgs a{};
    a.verdicts = h_verd;
    a.rejected = d_rej;
    if (dev) {
        std::vector<mv::Piece> pieces;
        for (unsigned h = 0; h <= mv::MAX_HEIGHT; h++)
            if (s.start[h + 1] > s.start[h]) pieces.push_back(mv::Piece{s.start[h], (uint32_t)(s.start[h + 1] - s.start[h]), h, 0});
        uint8_t *h_up = half[0];
        const unsigned wg = make_tabs(pieces, (MVerifyTab *)h_up, nullptr, nullptr);
        memcpy(h_up + TABS_BYTES, s.order.data(), 4 * k);
        memcpy(h_up + TABS_BYTES + mv::align256(4 * k), s.soff.data(), 4 * k);
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_up, stage_bytes, hipMemcpyHostToDevice, ctx->stream));
        a.roots = roots;
        a.vals = vals;
        a.sib = sib;
        a.dirs = dirs;
        a.order = (const uint32_t *)(d_stage + TABS_BYTES);
        a.soff = (const uint32_t *)(d_stage + TABS_BYTES + mv::align256(4 * k));
        launch_mverify((const MVerifyTab *)d_stage, (unsigned)pieces.size(), wg, a, true, pause_for(ctx, wg), ctx->stream);
    } else {
        if (chunks.size() > 1)
            for (int e = 0; e < 2; e++)
                if (!ctx->ev_verify[e]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_verify[e], hipEventDisableTiming));
        for (size_t ci = 0; ci < chunks.size(); ci++) {
            const mv::Chunk &c = chunks[ci];
            uint8_t *h_up = half[ci & 1];
            if (ci >= 2) HIPCHK(ctx, hipEventSynchronize(ctx->ev_verify[ci & 1]));  // the upload from this half has left it
            const uint8_t *d_chunk = d_stage + TABS_BYTES;
            const unsigned wg = make_tabs(c.pieces, (MVerifyTab *)h_up, d_chunk + c.off_sib, d_chunk + c.off_dirs);
            mv::stage_chunk(s, c, roots, vals, sib, dirs, h_up + TABS_BYTES, 8);
            // (the previous chunk's launch reads d_stage: the copy queues behind it on the stream)
            HIPCHK(ctx, hipMemcpyAsync(d_stage, h_up, TABS_BYTES + c.bytes, hipMemcpyHostToDevice, ctx->stream));
            if (chunks.size() > 1) HIPCHK(ctx, hipEventRecord(ctx->ev_verify[ci & 1], ctx->stream));
            a.order = (const uint32_t *)d_chunk;
            a.roots = d_chunk + c.off_roots;
            a.vals = (const uint64_t *)(d_chunk + c.off_vals);
            a.lo = c.lo;  // the descriptors hold sorted positions of the whole call
            launch_mverify((const MVerifyTab *)d_stage, (unsigned)c.pieces.size(), wg, a, false, pause_for(ctx, wg), ctx->stream);
        }
    }
    const DoneFlag done = done_flag(ctx, 2);
    launch_publish_u64(d_rej, 1, h_rej, true, ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    if (verdicts) memcpy(verdicts, h_verd, k);
    *n_rejected = (size_t)*h_rej;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// the argument checks both forms share; align: the device form's 16-byte roots / siblings and 8-byte values
zigz_status verify_args(zigz_ctx *ctx, size_t k, const uint8_t *roots, const size_t *heights, const uint64_t *vals,
                        const uint8_t *sib, const uint8_t *dirs, size_t *n_rejected, size_t *bad_index, bool align) {
    if (!ctx || !n_rejected) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_VERIFY_BATCH_MAX || !roots || !heights || !vals || !sib || !dirs) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (align && (((uintptr_t)roots | (uintptr_t)sib) & 15 || (uintptr_t)vals & 7)) return ZIGZ_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < k; i++)
        if (heights[i] > mv::MAX_HEIGHT) {
            set_err(ctx, "opening %zu has height %zu (at most %u)", i, heights[i], mv::MAX_HEIGHT);
            return fail_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        }
    return ZIGZ_OK;
}

}  // namespace

extern "C" zigz_status zigz_merkle_verify_batch(zigz_ctx *ctx, size_t k, const uint8_t *roots, const size_t *heights,
                                                const uint64_t *leaf_values, const uint8_t *siblings, const uint8_t *dirs,
                                                uint8_t *verdicts, size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    CHK(verify_args(ctx, k, roots, heights, leaf_values, siblings, dirs, n_rejected, bad_index, false));
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify_run(ctx, false, k, roots, heights, leaf_values, siblings, dirs, verdicts, n_rejected);
}

extern "C" zigz_status zigz_dev_merkle_verify_batch(zigz_ctx *ctx, size_t k, const uint8_t *d_roots, const size_t *heights,
                                                    const uint64_t *d_leaf_values, const uint8_t *d_siblings,
                                                    const uint8_t *d_dirs, uint8_t *verdicts, size_t *n_rejected,
                                                    size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    CHK(verify_args(ctx, k, d_roots, heights, d_leaf_values, d_siblings, d_dirs, n_rejected, bad_index, true));
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify_run(ctx, true, k, d_roots, heights, d_leaf_values, d_siblings, d_dirs, verdicts, n_rejected);
}
