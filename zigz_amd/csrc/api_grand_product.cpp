// C ABI of libzigz_hip.so, part 12: product trees and the batched grand-product argument.  The statement, the
// layout, the argument rules, the walk through the layers, the host's layers and the verifier's replay are
// grand_product_host.hpp's; the kernels grand_product.hip's.  Here: the schedules.
//   trees     every pass's descriptors and the tops' in ONE copy (from the staging region that outlives the call), then one
//             k_gp_layers launch per pass -- a column at layer J > 11 takes min(3, J - 11) levels -- and one k_gp_top launch;
//   prover    the trees of all instances into a workspace (the leaf layer is the caller's column), the top of every tree handed
//             off ONCE with the k_gp_top launch; layer 0 and the layers j <= 10 of all instances on the host's threads
//             (zc::tail_rounds under zc::Weight); then for j = 11 .. max v - 1 ONE sched::run over all instances with v_i > j, each
//             a zero-check family instance (M = 2, T = 1, alpha = 1, D = 2, tables L_j, H_j, tau^(j)) that starts from the
//             instance's transcript and hands it back;
//   verifier  A(leaf_point) of all proofs queued in the batched eval's launch first, the replays on the host's threads
//             meanwhile, combined after the hand-off.
#include "grand_product_host.hpp"
#include "zerocheck_family.hpp"

using namespace zk;

static_assert(gp::TOP_LOG2 == GP_TOP_LOG2 && gp::CHUNK == GP_CHUNK && gp::MAX_CHUNKS == MLE_BATCH_MAX_WGS, "header, host and kernels");
static_assert(GP_CHUNK == PRODUCT_CHUNK, "a layer's zero-check makes no more chunks than the tree's first pass");

namespace {

// the layer an instance's passes and its top start from: the column while nothing is built, then the tree buffer
inline const uint32_t *layer_ptr(const uint32_t *col, const uint32_t *tree, size_t n, unsigned j) {
    return ((size_t)1 << j) == n ? col : tree + gp::layer_at(n, j);
}

// Queues the trees of k columns (ns[i] powers of two >= 2, everything 16-byte aligned, the chunk limit checked by the callers).
// h_top != nullptr: the tops go to pinned memory too, column i's at word top_off[i], and `done` is signalled.
zigz_status trees_queue(zigz_ctx *ctx, size_t k, const uint32_t *const *cols, const size_t *ns, uint32_t *const *trees, uint32_t *h_top,
                        const size_t *top_off, DoneFlag done) {
    ZIGZ_NOTHROW_BEGIN
    struct Pass {
        size_t first, count, nwg;
    };
    std::vector<GpTab> tabs;
    std::vector<Pass> passes;
    std::vector<unsigned> J(k);
    for (size_t i = 0; i < k; i++) J[i] = log2_floor(ns[i]);
    for (;;) {
        Pass p{tabs.size(), 0, 0};
        for (size_t i = 0; i < k; i++) {
            const unsigned lv = gp::fused_levels(J[i]);
            if (!lv) continue;
            GpTab t{};
            t.in = layer_ptr(cols[i], trees[i], ns[i], J[i]);
            t.tree = trees[i];
            t.n = ns[i];
            t.log2_in = J[i];
            t.levels = lv;
            t.first_wg = (uint32_t)p.nwg;
            tabs.push_back(t);
            p.nwg += gp_wgs((size_t)1 << J[i]);
            p.count++;
            J[i] -= lv;
        }
        if (!p.count) break;
        passes.push_back(p);
    }
    const size_t top_at = align256(tabs.size() * sizeof(GpTab)), bytes = top_at + align256(k * sizeof(GpTop));
    uint8_t *h;
    void *d_stage;
    CHK(upload_region(ctx, bytes, &h));
    CHK(ws_get(ctx, WS_GP, bytes, &d_stage));
    if (!tabs.empty()) memcpy(h, tabs.data(), tabs.size() * sizeof(GpTab));
    GpTop *tops = (GpTop *)(h + top_at);
    for (size_t i = 0; i < k; i++) {
        GpTop t{};
        t.in = layer_ptr(cols[i], trees[i], ns[i], J[i]);
        t.tree = trees[i];
        t.n = ns[i];
        t.top_off = top_off ? top_off[i] : 0;
        t.log2_in = J[i];
        tops[i] = t;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_stage, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_open, ctx->stream));
    for (const Pass &p : passes) launch_gp_layers((const GpTab *)d_stage + p.first, (unsigned)p.count, (unsigned)p.nwg, ctx->stream);
    launch_gp_top((const GpTop *)((const uint8_t *)d_stage + top_at), (unsigned)k, h_top, ctx->stream, h_top ? done : DoneFlag());
    HIPCHK(ctx, hipGetLastError());
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

constexpr size_t DOWNLOAD_BYTES = (size_t)32 << 20;  // pinned staging per chunk of the host form's download

// Host form of the trees: the columns narrowed and uploaded in one copy, the trees built into a workspace one behind the other and
// brought back through pinned memory in chunks, widened on the way into the caller's arrays (word ns[i] - 1 is left alone)
zigz_status trees_host(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns, uint64_t *const *out, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    const std::vector<size_t> at = packed_offsets(ns, k);
    const size_t chunk = DOWNLOAD_BYTES / 4;
    uint8_t *pin;
    CHK(pinned(ctx, at[k] * 4, &pin));  // the narrowed columns on the way in, a chunk of the trees on the way out
    std::vector<const uint32_t *> cols;
    CHK(stage_host_tables(ctx, tables, ns, k, at, (uint32_t *)pin, WS_GP_IN, nullptr, cols, bad_index));
    void *d_trees;
    CHK(ws_get(ctx, WS_GP_TREE, at[k] * 4, &d_trees));
    std::vector<uint32_t *> trees(k);
    for (size_t i = 0; i < k; i++) trees[i] = (uint32_t *)d_trees + at[i];
    CHK(trees_queue(ctx, k, cols.data(), ns, trees.data(), nullptr, nullptr, DoneFlag()));
    const uint32_t *h = (const uint32_t *)pin;
    size_t first = 0;  // the first tree that reaches past the words already taken
    for (size_t lo = 0; lo < at[k]; lo += chunk) {
        const size_t hi = lo + chunk < at[k] ? lo + chunk : at[k];
        HIPCHK(ctx, hipMemcpyAsync(pin, (const uint32_t *)d_trees + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        while (first < k && at[first] + ns[first] <= lo) first++;
        for (size_t i = first; i < k && at[i] < hi; i++) {
            const size_t a = at[i] > lo ? at[i] : lo, end = at[i] + ns[i] - 1, b = end < hi ? end : hi;
            for (size_t x = a; x < b; x++) out[i][x - at[i]] = h[x - lo];
        }
    }
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// ---- the prover
zigz_status prove(zigz_ctx *ctx, const gp::ProveArgs &a, const uint32_t *const *d_tables, const uint64_t *const *h_tables,
                  uint64_t *products, uint64_t *layer_evals, uint64_t *rounds, uint64_t *points, uint64_t *layer_challenges,
                  uint64_t *leaf_points, uint64_t *leaf_evals, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    const size_t k = a.k;
    const size_t *ns = a.ns;
    const std::vector<size_t> at = packed_offsets(ns, k);
    std::vector<size_t> top_off(k + 1, 0);
    std::vector<unsigned> vs(k);
    unsigned max_v = 0;
    for (size_t i = 0; i < k; i++) {
        vs[i] = log2_floor(ns[i]);
        if (vs[i] > max_v) max_v = vs[i];
        top_off[i + 1] = top_off[i] + ((size_t)2 << (vs[i] < gp::TOP_LOG2 ? vs[i] : gp::TOP_LOG2));
    }
    // pinned: the tops | the narrowed columns of the host form
    const size_t tab_off = align256(top_off[k] * 4);
    uint8_t *pin;
    CHK(pinned(ctx, tab_off + (h_tables ? at[k] * 4 : 0), &pin));
    std::vector<const uint32_t *> up;
    if (h_tables) {
        CHK(stage_host_tables(ctx, h_tables, ns, k, at, (uint32_t *)(pin + tab_off), WS_GP_IN, nullptr, up, bad_index));
        d_tables = up.data();
    }
    void *d_trees;
    CHK(ws_get(ctx, WS_GP_TREE, at[k] * 4, &d_trees));
    std::vector<uint32_t *> trees(k);
    for (size_t i = 0; i < k; i++) trees[i] = (uint32_t *)d_trees + at[i];
    const DoneFlag done = done_flag(ctx, 2);
    CHK(trees_queue(ctx, k, d_tables, ns, trees.data(), (uint32_t *)pin, top_off.data(), done));
    CHK(wait_published(ctx, done));
    const uint32_t *h_top = (const uint32_t *)pin;
    for (size_t i = 0; i < k; i++)  // (a device column is not checked on the way in; the last word of a top is not written)
        for (size_t x = top_off[i]; x + 1 < top_off[i + 1]; x++)
            if (h_top[x] >= P) {
                set_err(ctx, "%s", NOT_CANONICAL_TEXT);
                return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
            }
    // the walks: layer 0 and the layers whose tables the host holds
    std::vector<gp::Walk> w(k);
    {
        size_t eoff = 0, roff = 0, poff = 0, voff = 0, foff = 0;
        for (size_t i = 0; i < k; i++) {
            const size_t v = vs[i];
            w[i].v = v;
            w[i].fixed = a.fixed ? a.fixed + foff : nullptr;
            w[i].product = products + i;
            w[i].layer_evals = layer_evals + eoff;
            w[i].rounds = rounds + roff;
            w[i].points = points + poff;
            w[i].layer_challenges = layer_challenges + voff;
            w[i].leaf_point = leaf_points + voff;
            w[i].leaf_eval = leaf_evals + i;
            eoff += gp::eval_words(v);
            roff += gp::round_words(v);
            poff += gp::point_words(v);
            voff += v;
            foff += gp::fixed_words(v);
        }
    }
    parallel_for(k, [&](size_t i) {
        const unsigned J = vs[i] < gp::TOP_LOG2 ? vs[i] : gp::TOP_LOG2;
        const uint32_t *top = h_top + top_off[i];
        auto layer = [&](unsigned j) { return top + (((size_t)2 << J) - ((size_t)2 << j)); };
        w[i].begin(*layer(0));
        for (unsigned j = 0; j < J; j++) gp::prove_host_layer(w[i], j, layer(j + 1));
    });
    for (const auto &x : w)
        if (x.st != ZIGZ_OK) return x.st;
    // the layers whose tables live on the device: one run of the zero-check schedule per layer, over every instance that has it
    for (unsigned j = gp::HOST_LAYER + 1; j < max_v; j++) {
        std::vector<size_t> who;
        for (size_t i = 0; i < k; i++)
            if (vs[i] > j) who.push_back(i);
        const size_t n = who.size(), m = (size_t)1 << j;
        std::vector<unsigned> n_tables(n, 2), n_terms(n, 1), degrees(n, 2);
        std::vector<uint8_t> idx(2 * n);
        std::vector<uint64_t> coeffs(n, 1), taus(n * j), fixed(a.fixed ? n * j : 0), claimed(n), lr(4 * (size_t)j * n), lp(n * j), evals(2 * n), eqs(n),
            finals(n);
        std::vector<const uint32_t *> tabs(2 * n);
        std::vector<size_t> lns(n, m);
        std::vector<Transcript> trs(n);
        for (size_t x = 0; x < n; x++) {
            const size_t i = who[x];
            idx[2 * x] = 0;
            idx[2 * x + 1] = 1;
            const uint32_t *next = layer_ptr(d_tables[i], trees[i], ns[i], j + 1);
            tabs[2 * x] = next;
            tabs[2 * x + 1] = next + m;
            memcpy(taus.data() + x * j, w[i].tau.data(), j * 8);
            if (a.fixed) memcpy(fixed.data() + x * j, w[i].fixed + gp::fixed_at(j), j * 8);
            trs[x] = w[i].tr;
        }
        const zc::Args za{{n, n_tables.data(), (const void *const *)tabs.data(), lns.data(), n_terms.data(), degrees.data(), idx.data(),
                           coeffs.data(), a.fixed ? fixed.data() : nullptr, claimed.data(), lr.data(), lp.data(), evals.data(), finals.data()},
                          taus.data(), eqs.data()};
        sched::ZeroCheck fam(za, evals.data(), eqs.data(), finals.data());
        size_t bad = 0;
        CHK(sched::run(ctx, fam, n, tabs.data(), nullptr, lns.data(), za.s.fixed, claimed.data(), lr.data(), lp.data(), &bad, trs.data()));
        for (size_t x = 0; x < n; x++) {
            gp::Walk &s = w[who[x]];
            memcpy(s.rounds + gp::rounds_at(j), lr.data() + 4 * (size_t)j * x, 4 * (size_t)j * 8);
            memcpy(s.points + gp::points_at(j), lp.data() + (size_t)j * x, (size_t)j * 8);
            s.tr = trs[x];
            s.layer_claim = claimed[x];
            s.close_layer(j, nullptr, evals[2 * x], evals[2 * x + 1]);
            if (s.st != ZIGZ_OK) return s.st;
        }
    }
    for (auto &x : w) x.finish();
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// ---- the verifier
zigz_status verify(zigz_ctx *ctx, const gp::VerifyArgs &a, bool host_tables, uint8_t *verdicts, uint64_t *expected_evals,
                   uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    if (a.k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    ZIGZ_NOTHROW_BEGIN
    const size_t k = a.k;
    const bool deferred = (a.flags & ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED) != 0;
    DoneFlag done;
    const uint64_t *oracle = nullptr;
    if (!deferred) CHK(mle_eval_pairs_queue(ctx, a.tables, host_tables, a.ns, k, a.leaf_points, false, nullptr, &oracle, &done, bad_index));
    std::vector<size_t> eoff(k + 1, 0), roff(k + 1, 0), voff(k + 1, 0);
    for (size_t i = 0; i < k; i++) {
        const size_t v = log2_floor(a.ns[i]);
        eoff[i + 1] = eoff[i] + gp::eval_words(v);
        roff[i + 1] = roff[i] + gp::round_words(v);
        voff[i + 1] = voff[i] + v;
    }
    // the k replays, underneath the evaluation
    std::vector<gp::Replay> rep(k);
    parallel_for(k, [&](size_t i) { rep[i] = gp::replay(a.products[i], a.layer_evals + eoff[i], a.rounds + roff[i], voff[i + 1] - voff[i]); });
    if (!deferred) CHK(wait_published(ctx, done));
    size_t rejected = 0;
    for (size_t i = 0; i < k; i++) {
        const uint8_t ok = gp::verdict(rep[i], a.leaf_points + voff[i], voff[i + 1] - voff[i], a.leaf_evals[i], deferred ? nullptr : oracle + i);
        rejected += !ok;
        if (verdicts) verdicts[i] = ok;
        if (expected_evals) expected_evals[i] = rep[i].expected;
        if (oracle_evals && !deferred) oracle_evals[i] = oracle[i];
    }
    *n_rejected = rejected;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_dev_product_layers_batch(zigz_ctx *ctx, size_t k, const uint32_t *const *d_tables, const size_t *ns,
                                                     uint32_t *const *d_out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(gp::check_layers_batch(gp::LayersArgs{k, (const void *const *)d_tables, ns, (const void *const *)d_out}, true, false, bad_index));
    if (gp::first_pass_chunks(ns, k) > gp::MAX_CHUNKS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    return trees_queue(ctx, k, d_tables, ns, d_out, nullptr, nullptr, DoneFlag());
}

extern "C" zigz_status zigz_product_layers_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns,
                                                 uint64_t *const *out, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(host_checks(ctx, tables, ns, k, bad_index, [&](size_t *f) {
        return gp::check_layers_batch(gp::LayersArgs{k, (const void *const *)tables, ns, (const void *const *)out}, false, false, f);
    }));
    if (gp::first_pass_chunks(ns, k) > gp::MAX_CHUNKS) return ZIGZ_ERR_INVALID_ARGUMENT;
    return trees_host(ctx, k, tables, ns, out, bad_index);
}

extern "C" zigz_status zigz_dev_grand_product_prove_batch(zigz_ctx *ctx, size_t k, const uint32_t *const *d_tables, const size_t *ns,
                                                          const uint64_t *fixed_challenges, uint64_t *products, uint64_t *layer_evals,
                                                          uint64_t *rounds, uint64_t *points, uint64_t *layer_challenges,
                                                          uint64_t *leaf_points, uint64_t *leaf_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const gp::ProveArgs a{k, (const void *const *)d_tables, ns, fixed_challenges, products, layer_evals, rounds, points, layer_challenges,
                          leaf_points, leaf_evals};
    CHK(gp::check_prove_batch(a, true, false, bad_index));
    if (gp::first_pass_chunks(ns, k) > gp::MAX_CHUNKS) return ZIGZ_ERR_INVALID_ARGUMENT;
    return prove(ctx, a, d_tables, nullptr, products, layer_evals, rounds, points, layer_challenges, leaf_points, leaf_evals, bad_index);
}

extern "C" zigz_status zigz_grand_product_prove_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns,
                                                      const uint64_t *fixed_challenges, uint64_t *products, uint64_t *layer_evals,
                                                      uint64_t *rounds, uint64_t *points, uint64_t *layer_challenges, uint64_t *leaf_points,
                                                      uint64_t *leaf_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const gp::ProveArgs a{k, (const void *const *)tables, ns, fixed_challenges, products, layer_evals, rounds, points, layer_challenges,
                          leaf_points, leaf_evals};
    CHK(host_checks(ctx, tables, ns, k, bad_index, [&](size_t *f) { return gp::check_prove_batch(a, false, false, f); }));
    if (gp::first_pass_chunks(ns, k) > gp::MAX_CHUNKS) return ZIGZ_ERR_INVALID_ARGUMENT;
    return prove(ctx, a, nullptr, tables, products, layer_evals, rounds, points, layer_challenges, leaf_points, leaf_evals, bad_index);
}

extern "C" zigz_status zigz_dev_grand_product_verify_batch(zigz_ctx *ctx, size_t k, const uint32_t *const *d_tables, const size_t *ns,
                                                           const uint64_t *products, const uint64_t *layer_evals, const uint64_t *rounds,
                                                           const uint64_t *leaf_points, const uint64_t *leaf_evals, uint32_t flags,
                                                           uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                           size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const gp::VerifyArgs a{k, (const void *const *)d_tables, ns, products, layer_evals, rounds, leaf_points, leaf_evals, flags, n_rejected};
    CHK(gp::check_verify_batch(a, true, false, bad_index));
    return verify(ctx, a, false, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_grand_product_verify_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns,
                                                       const uint64_t *products, const uint64_t *layer_evals, const uint64_t *rounds,
                                                       const uint64_t *leaf_points, const uint64_t *leaf_evals, uint32_t flags,
                                                       uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                       size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const gp::VerifyArgs a{k, (const void *const *)tables, ns, products, layer_evals, rounds, leaf_points, leaf_evals, flags, n_rejected};
    if (tables && k && !(flags & ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED)) {
        CHK(host_checks(ctx, tables, ns, k, bad_index, [&](size_t *f) { return gp::check_verify_batch(a, false, false, f); }));
    } else {
        CHK(gp::check_verify_batch(a, false, false, bad_index));
    }
    return verify(ctx, a, true, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}
