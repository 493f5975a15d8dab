// C ABI of libzigz_hip.so, part 8: batched MLE evaluation over free-standing tables and batched sumcheck verification on top of
// it.
//
// Schedule of one call: the host writes the k descriptors and the 2 v factors of every point (1 - r and r, Montgomery form)
// into pinned memory and queues ONE copy of them, ONE launch that evaluates all k pairs (mle_batch.hip: exact u64 sums, one
// partial per workgroup) and one small launch that adds each pair's partials, reduces mod p into pinned memory and stores the
// completion word.  The host polls that word: no stream synchronisation on the normal path.  The verify entries
// queue the same copy and two launches over the proofs' final points, replay the k transcripts on the host's threads while the GPU
// evaluates (the evaluation point comes from the proof, not from the transcript, so neither waits for the other), and combine
// the two after the hand-off.  The argument checks and the replay are plain host code: sumcheck_verify_host.hpp.
#include "api_internal.hpp"
#include "sumcheck_verify_host.hpp"

using namespace zk;

// The k descriptors of one eval launch and the factor pairs of its points (1 - r and r, Montgomery form), pair i's at f + 2 (sum
// of the variables before it); returns the launch's workgroup count.  points: the pairs' coordinates one behind the other.
// reversed: index bit v is bound to the point's coordinate nv - 1 - v instead of v (the order of the descriptor's factors).
size_t mle_batch_fill(const uint32_t *const *d_tables, const size_t *ns, size_t k, const uint64_t *points, bool reversed,
                      MleBatchTab *tab, uint32_t *f) {
    size_t off = 0, wg = 0;
    for (size_t i = 0; i < k; i++) {
        const unsigned nv = log2_floor(ns[i]);
        MleBatchTab t{};
        t.vals = d_tables[i];
        t.n = ns[i];
        t.nv = nv;
        t.first_wg = (uint32_t)wg;
        t.f_off = (uint32_t)(2 * off);
        t.slot = (uint32_t)i;
        tab[i] = t;
        for (unsigned v = 0; v < nv; v++) {
            const uint64_t r = points[off + (reversed ? nv - 1 - v : v)];
            f[2 * (off + v)] = host_to_mont(f_sub(1, r));
            f[2 * (off + v) + 1] = host_to_mont(r);
        }
        off += nv;
        wg += (ns[i] + MLE_BATCH_CHUNK - 1) / MLE_BATCH_CHUNK;
    }
    return wg;
}

namespace {

// one call's pinned region: results (k u64) | descriptors | factors | the narrowed tables of the host forms
struct Layout {
    size_t k = 0, tot_v = 0, nwg = 0;
    size_t desc_off = 0, f_off = 0, stage_bytes = 0, tab_off = 0, tab_words = 0, bytes = 0;
    std::vector<size_t> at;  // host forms: table i's first word among the narrowed tables (every table 16-byte aligned)
};

// ns[i] are powers of two <= 2^32 (checked by the callers)
zigz_status plan(const size_t *ns, size_t k, bool host_tables, Layout &L) {
    L.k = k;
    for (size_t i = 0; i < k; i++) {
        L.tot_v += log2_floor(ns[i]);
        L.nwg += (ns[i] + MLE_BATCH_CHUNK - 1) / MLE_BATCH_CHUNK;
    }
    if (L.nwg > MLE_BATCH_MAX_WGS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    L.desc_off = align256(k * 8);
    L.f_off = L.desc_off + align256(k * sizeof(MleBatchTab));
    L.stage_bytes = L.f_off + align256(2 * L.tot_v * 4 + 4) - L.desc_off;
    L.tab_off = L.desc_off + L.stage_bytes;
    if (host_tables) {
        L.at = packed_offsets(ns, k);
        L.tab_words = L.at[k];
    }
    L.bytes = L.tab_off + L.tab_words * 4;
    return ZIGZ_OK;
}

// Queues the copy and the two launches; the k results arrive as u64 at the start of `pin` once `done` is published.
zigz_status eval_queue(zigz_ctx *ctx, const Layout &L, uint8_t *pin, const uint32_t *const *d_tables, const size_t *ns,
                       const uint64_t *points, bool reversed, DoneFlag *done) {
    void *d_stage, *d_part;
    CHK(ws_get(ctx, WS_MLEBATCH, L.stage_bytes, &d_stage));
    CHK(ws_get(ctx, WS_MLEBATCH_PART, L.nwg * 8, &d_part));  // one partial sum per workgroup, all written by the launch
    mle_batch_fill(d_tables, ns, L.k, points, reversed, (MleBatchTab *)(pin + L.desc_off), (uint32_t *)(pin + L.f_off));
    HIPCHK(ctx, hipMemcpyAsync(d_stage, pin + L.desc_off, L.stage_bytes, hipMemcpyHostToDevice, ctx->stream));
    *done = done_flag(ctx, 2);
    const uint8_t *ds = (const uint8_t *)d_stage;
    launch_mle_batch_eval((const MleBatchTab *)ds, (unsigned)L.k, (unsigned)L.nwg, (const uint32_t *)(ds + (L.f_off - L.desc_off)),
                          (unsigned long long *)d_part, ctx->stream);
    launch_mle_batch_finish((const MleBatchTab *)ds, (unsigned)L.k, (const unsigned long long *)d_part, (uint64_t *)pin, ctx->stream,
                            *done);
    HIPCHK(ctx, hipGetLastError());
    return ZIGZ_OK;
}

zigz_status eval_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const uint64_t *const *h_tables, const size_t *ns, size_t k,
                       const uint64_t *points, uint64_t *out, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    Layout L;
    CHK(plan(ns, k, h_tables != nullptr, L));
    uint8_t *pin;
    CHK(pinned(ctx, L.bytes, &pin));
    std::vector<const uint32_t *> d;
    if (h_tables) {
        CHK(stage_host_tables(ctx, h_tables, ns, k, L.at, (uint32_t *)(pin + L.tab_off), WS_MLEBATCH_IN, nullptr, d, bad_index));
        d_tables = d.data();
    }
    DoneFlag done;
    CHK(eval_queue(ctx, L, pin, d_tables, ns, points, false, &done));
    CHK(wait_published(ctx, done));
    memcpy(out, pin, k * 8);
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

zigz_status verify_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const uint64_t *const *h_tables, const size_t *ns,
                         size_t k, const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                         const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts, uint64_t *expected_evals,
                         uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    Layout L;
    CHK(plan(ns, k, h_tables != nullptr, L));
    uint8_t *pin;
    CHK(pinned(ctx, L.bytes, &pin));
    std::vector<const uint32_t *> d;
    if (h_tables) {
        CHK(stage_host_tables(ctx, h_tables, ns, k, L.at, (uint32_t *)(pin + L.tab_off), WS_MLEBATCH_IN, nullptr, d, bad_index));
        d_tables = d.data();
    }
    DoneFlag done;
    CHK(eval_queue(ctx, L, pin, d_tables, ns, points, (flags & ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED) != 0, &done));
    // the k replays, underneath the evaluation
    std::vector<size_t> voff(k + 1, 0);
    for (size_t i = 0; i < k; i++) voff[i + 1] = voff[i] + log2_floor(ns[i]);
    std::vector<sv::Replay> rep(k);
    parallel_for(k, [&](size_t i) { rep[i] = sv::replay_rounds(claimed_sums[i], rounds + 2 * voff[i], voff[i + 1] - voff[i]); });
    CHK(wait_published(ctx, done));
    const uint64_t *ev = (const uint64_t *)pin;
    size_t rejected = 0;
    for (size_t i = 0; i < k; i++) {
        const uint8_t ok = sv::verdict(rep[i], ev[i], final_evals[i]);
        rejected += !ok;
        if (verdicts) verdicts[i] = ok;
        if (expected_evals) expected_evals[i] = rep[i].expected;
        if (oracle_evals) oracle_evals[i] = ev[i];
    }
    *n_rejected = rejected;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_dev_mle_eval_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k,
                                               const uint64_t *points, uint64_t *out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(sv::check_eval_batch((const void *const *)d_tables, ns, k, points, out, true, false, bad_index));
    return eval_batch(ctx, d_tables, nullptr, ns, k, points, out, bad_index);
}

extern "C" zigz_status zigz_mle_eval_batch(zigz_ctx *ctx, const uint64_t *const *tables, const size_t *ns, size_t k,
                                           const uint64_t *points, uint64_t *out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(host_checks(ctx, tables, ns, k, bad_index, [&](size_t *f) {
        return sv::check_eval_batch((const void *const *)tables, ns, k, points, out, false, false, f);
    }));
    return eval_batch(ctx, nullptr, tables, ns, k, points, out, bad_index);
}

extern "C" zigz_status zigz_dev_sumcheck_verify_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k,
                                                      const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                                                      const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                                      uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                      size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    CHK(sv::check_verify_batch((const void *const *)d_tables, ns, k, claimed_sums, rounds, points, final_evals, flags, n_rejected,
                               true, false, bad_index));
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify_batch(ctx, d_tables, nullptr, ns, k, claimed_sums, rounds, points, final_evals, flags, verdicts, expected_evals,
                        oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_sumcheck_verify_batch(zigz_ctx *ctx, const uint64_t *const *tables, const size_t *ns, size_t k,
                                                  const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                                                  const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                                  uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                  size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    CHK(host_checks(ctx, tables, ns, k, bad_index, [&](size_t *f) {
        return sv::check_verify_batch((const void *const *)tables, ns, k, claimed_sums, rounds, points, final_evals, flags,
                                      n_rejected, false, false, f);
    }));
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify_batch(ctx, nullptr, tables, ns, k, claimed_sums, rounds, points, final_evals, flags, verdicts, expected_evals,
                        oracle_evals, n_rejected, bad_index);
}
