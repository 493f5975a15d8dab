// C ABI of libzigz_hip.so, part 8: batched MLE evaluation over free-standing tables and batched sumcheck verification on top of
// it; batched eq tables and the verification of product proofs, whose table factors go through the same eval
// launch.
//
// Schedule of one call: the host writes the k descriptors and the 2 v factors of every point (1 - r and r, Montgomery form)
// into pinned memory and queues ONE copy of them, ONE launch that evaluates all k pairs (mle_batch.hip: exact u64 sums, one
// partial per workgroup) and one small launch that adds each pair's partials, reduces mod p into pinned memory and stores the
// completion word.  The host polls that word: no stream synchronisation on the normal path.  The verify entries
// queue the same copy and two launches over the proofs' final points, replay the k transcripts on the host's threads while the GPU
// evaluates (the evaluation point comes from the proof, not from the transcript, so neither waits for the other), and combine
// the two after the hand-off.  The argument checks and the replay are plain host code: sumcheck_verify_host.hpp.
//
// The product verifier is the same schedule over one (table, point) pair per TABLE factor of every proof; a factor eq(tau, .) is
// v multiplications on the host next to the replay and never a table.  The eq tables are one copy (descriptors and factor pairs)
// and one launch (eq_batch.hip) that the device form leaves queued.  Checks, replay, eq_at, verdict: product_verify_host.hpp.
#include "api_internal.hpp"
#include "product_verify_host.hpp"

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

// m (table, point) pairs of a verifier through the eval's copy and two launches (the product and sum-of-products verifiers: one
// pair per table oracle of every proof): host tables are narrowed and uploaded first (a value >= p: ZIGZ_ERR_NOT_CANONICAL with
// owner[pair] in *bad_index).  The m values are at *results once `done` is published.  m == 0 queues nothing.
zigz_status mle_eval_pairs_queue(zigz_ctx *ctx, const void *const *tables, bool host_tables, const size_t *ns, size_t m,
                                 const uint64_t *points, bool reversed, const size_t *owner, const uint64_t **results, DoneFlag *done,
                                 size_t *bad_index) {
    Layout L;
    CHK(plan(ns, m, host_tables, L));
    if (!m) return ZIGZ_OK;
    uint8_t *pin;
    CHK(pinned(ctx, L.bytes, &pin));
    std::vector<const uint32_t *> d;
    if (host_tables) {
        CHK(stage_host_tables(ctx, (const uint64_t *const *)tables, ns, m, L.at, (uint32_t *)(pin + L.tab_off), WS_MLEBATCH_IN, owner, d,
                              bad_index));
    } else {
        d.assign((const uint32_t *const *)tables, (const uint32_t *const *)tables + m);
    }
    *results = (const uint64_t *)pin;
    return eval_queue(ctx, L, pin, d.data(), ns, points, reversed, done);
}

namespace {

// ---- product proofs: the oracles are the proofs' factors, a table (one pair of the eval launch) or eq(tau, .) (host, closed form)
zigz_status verify_product_batch(zigz_ctx *ctx, const pv::VerifyArgs &a, bool host_tables, uint8_t *verdicts,
                                 uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    const size_t k = a.k;
    const bool reversed = (a.flags & ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED) != 0;
    // per proof: its first factor, variable, round word and tau word; per table factor: one pair of the eval launch
    std::vector<size_t> foff(k + 1, 0), voff(k + 1, 0), roff(k + 1, 0), eoff(k + 1, 0);
    std::vector<const void *> tabs;
    std::vector<size_t> pair_ns, owner, pair_of;
    std::vector<uint64_t> pair_points;
    for (size_t i = 0; i < k; i++) {
        const unsigned d = a.degrees[i];
        const size_t v = log2_floor(a.ns[i]);
        size_t neq = 0;
        for (unsigned j = 0; j < d; j++) {
            if (pv::kind_of(a, foff[i] + j) == pv::KIND_EQ) {
                neq++;
                pair_of.push_back((size_t)-1);
                continue;
            }
            pair_of.push_back(tabs.size());
            tabs.push_back(a.factors[foff[i] + j]);
            pair_ns.push_back(a.ns[i]);
            owner.push_back(i);
            pair_points.insert(pair_points.end(), a.points + voff[i], a.points + voff[i] + v);
        }
        foff[i + 1] = foff[i] + d;
        voff[i + 1] = voff[i] + v;
        roff[i + 1] = roff[i] + (size_t)(d + 1) * v;
        eoff[i + 1] = eoff[i] + neq * v;
    }
    const size_t m = tabs.size();
    DoneFlag done;
    const uint64_t *pairs = nullptr;
    CHK(mle_eval_pairs_queue(ctx, tabs.data(), host_tables, pair_ns.data(), m, pair_points.data(), reversed, owner.data(), &pairs, &done,
                             bad_index));
    // the k replays and the eq factors, underneath the evaluation
    std::vector<sv::Replay> rep(k);
    std::vector<uint64_t> ev(foff[k], 0);
    parallel_for(k, [&](size_t i) {
        const size_t v = voff[i + 1] - voff[i];
        rep[i] = pv::replay_rounds(a.claimed_sums[i], a.rounds + roff[i], v, a.degrees[i]);
        const uint64_t *tau = a.eq_points ? a.eq_points + eoff[i] : nullptr;
        for (size_t f = foff[i]; f < foff[i + 1]; f++)
            if (pair_of[f] == (size_t)-1) {
                ev[f] = pv::eq_at(tau, a.points + voff[i], v, reversed);
                tau += v;
            }
    });
    if (m) CHK(wait_published(ctx, done));
    size_t rejected = 0;
    for (size_t i = 0; i < k; i++) {
        for (size_t f = foff[i]; f < foff[i + 1]; f++)
            if (pair_of[f] != (size_t)-1) ev[f] = pairs[pair_of[f]];
        const uint8_t ok = pv::verdict(rep[i], ev.data() + foff[i], a.degrees[i], a.final_evals[i],
                                       a.factor_evals ? a.factor_evals + foff[i] : nullptr);
        rejected += !ok;
        if (verdicts) verdicts[i] = ok;
        if (expected_evals) expected_evals[i] = rep[i].expected;
    }
    if (oracle_evals) memcpy(oracle_evals, ev.data(), foff[k] * 8);
    *n_rejected = rejected;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// ---- eq tables
constexpr size_t EQ_DOWNLOAD_BYTES = (size_t)32 << 20;  // pinned staging per chunk of the host form's download

inline size_t eq_chunks(const size_t *ns, size_t k) {
    size_t nwg = 0;
    for (size_t i = 0; i < k; i++) nwg += (ns[i] + MLE_BATCH_CHUNK - 1) / MLE_BATCH_CHUNK;
    return nwg;
}

// One copy (descriptors | factor pairs, from the staging region that outlives the call) and one launch, left queued on the
// context's stream.  ns[i] are powers of two <= 2^32, d_out[i] 16-byte aligned, the tables together at most MLE_BATCH_MAX_WGS
// chunks (checked by the callers).
zigz_status eq_queue(zigz_ctx *ctx, size_t k, const size_t *ns, const uint64_t *points, uint32_t *const *d_out) {
    size_t tot_v = 0;
    for (size_t i = 0; i < k; i++) tot_v += log2_floor(ns[i]);
    const size_t nwg = eq_chunks(ns, k);
    const size_t f_off = align256(k * sizeof(EqBatchTab)), bytes = f_off + align256(2 * tot_v * 4 + 4);
    uint8_t *h;
    void *d_stage;
    CHK(upload_region(ctx, bytes, &h));
    CHK(ws_get(ctx, WS_EQ, bytes, &d_stage));
    EqBatchTab *tab = (EqBatchTab *)h;
    uint32_t *f = (uint32_t *)(h + f_off);
    size_t off = 0, wg = 0;
    for (size_t i = 0; i < k; i++) {
        const unsigned nv = log2_floor(ns[i]);
        EqBatchTab t{};
        t.out = d_out[i];
        t.n = ns[i];
        t.nv = nv;
        t.first_wg = (uint32_t)wg;
        t.f_off = (uint32_t)(2 * off);
        tab[i] = t;
        for (unsigned v = 0; v < nv; v++) {
            f[2 * (off + v)] = host_to_mont(f_sub(1, points[off + v]));
            f[2 * (off + v) + 1] = host_to_mont(points[off + v]);
        }
        off += nv;
        wg += (ns[i] + MLE_BATCH_CHUNK - 1) / MLE_BATCH_CHUNK;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_stage, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_open, ctx->stream));
    launch_eq_batch_expand((const EqBatchTab *)d_stage, (unsigned)k, (unsigned)nwg, (const uint32_t *)((const uint8_t *)d_stage + f_off),
                           ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return ZIGZ_OK;
}

// Host form: the tables are built into a workspace, one behind the other (every table 16-byte aligned), and come back through
// pinned memory in chunks of at most EQ_DOWNLOAD_BYTES, widened to u64 on the way into the caller's arrays.
zigz_status eq_host(zigz_ctx *ctx, size_t k, const size_t *ns, const uint64_t *points, uint64_t *const *out) {
    ZIGZ_NOTHROW_BEGIN
    const std::vector<size_t> at = packed_offsets(ns, k);
    void *d_tabs;
    CHK(ws_get(ctx, WS_EQ_OUT, at[k] * 4, &d_tabs));
    std::vector<uint32_t *> d(k);
    for (size_t i = 0; i < k; i++) d[i] = (uint32_t *)d_tabs + at[i];
    CHK(eq_queue(ctx, k, ns, points, d.data()));
    const size_t chunk = EQ_DOWNLOAD_BYTES / 4;
    uint8_t *pin;
    CHK(pinned(ctx, (at[k] < chunk ? at[k] : chunk) * 4, &pin));
    const uint32_t *h = (const uint32_t *)pin;
    size_t first = 0;  // the first table that reaches past the words already taken
    for (size_t lo = 0; lo < at[k]; lo += chunk) {
        const size_t hi = lo + chunk < at[k] ? lo + chunk : at[k];
        HIPCHK(ctx, hipMemcpyAsync(pin, (const uint32_t *)d_tabs + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        while (first < k && at[first] + ns[first] <= lo) first++;
        for (size_t i = first; i < k && at[i] < hi; i++) {
            const size_t a = at[i] > lo ? at[i] : lo, b = at[i] + ns[i] < hi ? at[i] + ns[i] : hi;
            for (size_t x = a; x < b; x++) out[i][x - at[i]] = h[x - lo];
        }
    }
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

extern "C" zigz_status zigz_dev_sumcheck_verify_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                                              const uint32_t *const *d_factors, const uint8_t *factor_kinds,
                                                              const uint64_t *eq_points, const size_t *ns, const uint64_t *claimed_sums,
                                                              const uint64_t *rounds, const uint64_t *points,
                                                              const uint64_t *factor_evals, const uint64_t *final_evals, uint32_t flags,
                                                              uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                              size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const pv::VerifyArgs a{k, degrees, (const void *const *)d_factors, factor_kinds, eq_points, ns, claimed_sums, rounds, points,
                           factor_evals, final_evals, flags, n_rejected};
    CHK(pv::check_verify_product_batch(a, true, false, bad_index));
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify_product_batch(ctx, a, false, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_sumcheck_verify_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                                          const uint64_t *const *factors, const uint8_t *factor_kinds,
                                                          const uint64_t *eq_points, const size_t *ns, const uint64_t *claimed_sums,
                                                          const uint64_t *rounds, const uint64_t *points, const uint64_t *factor_evals,
                                                          const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                                          uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                          size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const pv::VerifyArgs a{k, degrees, (const void *const *)factors, factor_kinds, eq_points, ns, claimed_sums, rounds, points,
                           factor_evals, final_evals, flags, n_rejected};
    bool value = false;
    const zigz_status st = pv::check_verify_product_batch_host(a, bad_index, &value);
    if (value) set_err(ctx, "%s", NOT_CANONICAL_TEXT);
    CHK(st);
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify_product_batch(ctx, a, true, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_dev_eq_table_batch(zigz_ctx *ctx, size_t k, const size_t *ns, const uint64_t *points,
                                               uint32_t *const *d_out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(pv::check_eq_table_batch(k, ns, points, (const void *const *)d_out, true, bad_index));
    if (eq_chunks(ns, k) > MLE_BATCH_MAX_WGS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    return eq_queue(ctx, k, ns, points, d_out);
}

extern "C" zigz_status zigz_eq_table_batch(zigz_ctx *ctx, size_t k, const size_t *ns, const uint64_t *points, uint64_t *const *out,
                                           size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(pv::check_eq_table_batch(k, ns, points, (const void *const *)out, false, bad_index));
    if (eq_chunks(ns, k) > MLE_BATCH_MAX_WGS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    return eq_host(ctx, k, ns, points, out);
}
