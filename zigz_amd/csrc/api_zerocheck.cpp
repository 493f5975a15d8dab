// C ABI of libzigz_hip.so, part 11: the zero-check sumcheck with the eq factor in closed form and its verifier.
//
// The prover's schedule is api_sop.cpp's over a pool WITHOUT eq: per round one copy of the live instances' descriptors, one data
// pass (k_zc_sums, then k_zc_bind) and the sop finish launch; the host turns the class sums into the D + 1 coefficients of t_r
// (sop_host.hpp: coefficients), multiplies by the round's linear factor and the prefix scalar (zerocheck_host.hpp: Weight) and
// steps every live transcript on its threads with D + 2 coefficients.  What is new in the copies: behind every descriptor goes the
// instance's ZcWeights (two pointers), and the FIRST copy also carries the weights themselves -- per live instance the 1024 words
// of lo and the stages of hi, fewer than 2^(v - 10) words (zerocheck_host.hpp: build_weights) --, which stay where they are for
// the rest of the call: a round only points at its stage.  The tails are handed over by the sop launch and finished by
// zc::tail_rounds.  The workspaces are the product prover's: calls on a context are serial.
//
// The verifier replays the rounds on the host's threads while the batched eval's launch (api_mle_batch.cpp) evaluates every pool
// table once; eq(tau, q) is a closed form on the host.
#include "api_internal.hpp"
#include "zerocheck_host.hpp"

using namespace zk;

static_assert(sop::MAX_TABLES == SOP_MAX_TABLES && sop::MAX_TERMS == SOP_MAX_TERMS && sop::SUMS == SOP_SUMS, "header, host and kernels");
static_assert(zc::LOG2_LO == ZC_LOG2_LO && pd::R1 == R_MOD_P, "the host builds the weights the way the kernels split and multiply them");
static_assert(sizeof(SopTab) % alignof(ZcWeights) == 0, "the weights' pointers go right behind the descriptors");

namespace {

constexpr size_t LO_WORDS = (size_t)1 << ZC_LOG2_LO;

struct Inst {
    size_t len = 0, tail_off = 0;
    const uint32_t *cur[SOP_MAX_TABLES] = {};
    uint32_t *work[SOP_MAX_TABLES] = {};
    SopTerm term[SOP_MAX_TERMS] = {};  // sorted by degree, as the kernels walk them
    unsigned n_deg[PRODUCT_MAX_DEGREE] = {};
    uint64_t ch = 0;      // the challenge of the instance's last round
    size_t w_off = 0;     // live: first word of its weights (lo, then the stages of hi) in the weights region
    SumcheckRounds pr;
    zc::Weight w;
};

// a live instance's words in the weights region: lo and the stages of hi, rounded up so that the next lo is 16-byte aligned
size_t weight_words(size_t n) { return LO_WORDS + (((size_t)1 << (log2_floor(n) - ZC_LOG2_LO)) + 3) / 4 * 4; }

// one call's pinned region: sums (SOP_SUMS u64 per instance) | tails (u32) | round descriptors + weight pointers | weights | tail
// descriptors | the narrowed tables of the host form.  The device staging holds descriptors | weights | tail descriptors | partials.
struct Layout {
    size_t tail_off = 0, tail_words = 0, desc_off = 0, desc_bytes = 0, w_off = 0, w_bytes = 0, tdesc_off = 0, tdesc_bytes = 0, tab_off = 0,
           tab_words = 0, bytes = 0;
    size_t nwg = 0, work_words = 0;  // workgroups of round 0; words of all bound copies
    std::vector<size_t> fns, owner;  // every pool table's length and instance
    std::vector<size_t> at;          // host form: table f's first word among the narrowed tables (each 16-byte aligned)
};

zigz_status plan(size_t k, const unsigned *n_tables, const size_t *ns, bool host_tables, Layout &L) {
    size_t w_words = 0;
    for (size_t i = 0; i < k; i++) {
        L.tail_words += n_tables[i] * (ns[i] < HOST_TAIL_MAX ? ns[i] : HOST_TAIL_MAX);
        if (ns[i] > HOST_TAIL_MAX) {
            L.nwg += product_wgs(ns[i]);
            L.work_words += n_tables[i] * (ns[i] / 2);
            w_words += weight_words(ns[i]);
        }
        L.fns.insert(L.fns.end(), n_tables[i], ns[i]);
        L.owner.insert(L.owner.end(), n_tables[i], i);
    }
    if (L.nwg > MLE_BATCH_MAX_WGS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    L.desc_bytes = align256(k * (sizeof(SopTab) + sizeof(ZcWeights)));
    L.w_bytes = align256(w_words * 4);
    L.tdesc_bytes = align256(k * sizeof(SopTab));
    L.tail_off = align256(k * SOP_SUMS * 8);
    L.desc_off = L.tail_off + align256(L.tail_words * 4);
    L.w_off = L.desc_off + L.desc_bytes;
    L.tdesc_off = L.w_off + L.w_bytes;
    L.tab_off = L.tdesc_off + L.tdesc_bytes;
    if (host_tables) {
        L.at = packed_offsets(L.fns.data(), L.fns.size());
        L.tab_words = L.at[L.fns.size()];
    }
    L.bytes = L.tab_off + L.tab_words * 4;
    return ZIGZ_OK;
}

zigz_status run(zigz_ctx *ctx, const zc::Args &za, const uint32_t *const *d_tables, const uint64_t *const *h_tables,
                uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals,
                uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    const sop::Args &a = za.s;
    const size_t k = a.k;
    Layout L;
    CHK(plan(k, a.n_tables, a.ns, h_tables != nullptr, L));
    uint8_t *pin;
    CHK(pinned(ctx, L.bytes, &pin));
    std::vector<const uint32_t *> up;
    if (h_tables) {
        CHK(stage_host_tables(ctx, h_tables, L.fns.data(), L.fns.size(), L.at, (uint32_t *)(pin + L.tab_off), WS_PRODUCT_IN,
                              L.owner.data(), up, bad_index));
        d_tables = up.data();
    }
    void *d_stage, *d_work;
    CHK(ws_get(ctx, WS_PRODUCT, L.desc_bytes + L.w_bytes + L.tdesc_bytes + L.nwg * SOP_SUMS * 8, &d_stage));
    CHK(ws_get(ctx, WS_PRODUCT_WORK, L.work_words * 4, &d_work));
    const SopTab *d_desc = (const SopTab *)d_stage, *d_tdesc = (const SopTab *)((uint8_t *)d_stage + L.desc_bytes + L.w_bytes);
    const uint32_t *d_weights = (const uint32_t *)((uint8_t *)d_stage + L.desc_bytes);
    unsigned long long *d_part = (unsigned long long *)((uint8_t *)d_stage + L.desc_bytes + L.w_bytes + L.tdesc_bytes);
    SopTab *h_desc = (SopTab *)(pin + L.desc_off), *h_tdesc = (SopTab *)(pin + L.tdesc_off);
    uint32_t *h_weights = (uint32_t *)(pin + L.w_off);
    const uint64_t *h_sums = (const uint64_t *)pin;

    const std::vector<sop::Shape> sh = sop::shapes(k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs);
    const std::vector<size_t> roff = zc::round_offsets(sh);
    std::vector<Inst> t(k);
    std::vector<size_t> live, next;
    {
        size_t woff = 0, toff = 0, wwoff = 0;
        for (size_t i = 0; i < k; i++) {
            Inst &s = t[i];
            const sop::Shape &h = sh[i];
            s.len = a.ns[i];
            s.tail_off = toff;
            toff += h.M * (a.ns[i] < HOST_TAIL_MAX ? a.ns[i] : HOST_TAIL_MAX);
            for (unsigned j = 0; j < h.M; j++) {
                s.cur[j] = d_tables[h.moff + j];
                if (a.ns[i] > HOST_TAIL_MAX) {  // every table's bound copy is 16-byte aligned: n / 2 >= 1024 words
                    s.work[j] = (uint32_t *)d_work + woff;
                    woff += a.ns[i] / 2;
                }
            }
            unsigned nt = 0;
            for (unsigned d = 1; d <= PRODUCT_MAX_DEGREE; d++)
                for (unsigned x = 0; x < h.T; x++)
                    if (h.terms[x].d == d) {
                        s.term[nt++] = SopTerm{sop_term_word(d, h.terms[x].idx), host_to_mont(h.terms[x].alpha)};
                        s.n_deg[d - 1]++;
                    }
            s.pr.ncoef = h.D + 2;
            s.pr.nv = h.nv;
            s.pr.claimed_sum = claimed_sums + i;
            s.pr.rounds = rounds + roff[i];
            s.pr.point = points + h.voff;
            s.pr.fixed = a.fixed ? a.fixed + h.voff : nullptr;
            s.w.tau = za.eq_points + h.voff;
            s.w.v = h.nv;
            if (a.ns[i] > HOST_TAIL_MAX) {
                s.w_off = wwoff;
                wwoff += weight_words(a.ns[i]);
                live.push_back(i);
            }
        }
    }
    // the live instances' weights, behind the descriptors of the first copy
    parallel_for(live.size(), [&](size_t x) {
        const Inst &s = t[live[x]];
        zc::build_weights(s.w.tau, (unsigned)s.w.v, ZC_LOG2_LO, h_weights + s.w_off, h_weights + s.w_off + LO_WORDS);
    });
    // instance i's descriptor with its current tables
    auto describe = [&](size_t i) {
        const Inst &s = t[i];
        SopTab p{};
        for (unsigned j = 0; j < sh[i].M; j++) p.in[j] = s.cur[j];
        for (unsigned x = 0; x < sh[i].T; x++) p.term[x] = s.term[x];
        p.m = s.len;
        p.n_tables = sh[i].M;
        p.n_terms = sh[i].T;
        p.n_d1 = s.n_deg[0];
        p.n_d2 = s.n_deg[1];
        return p;
    };
    // the live instances' descriptors and weight pointers for one pass; returns its workgroup count.  The pass sums for the round
    // with `pairs` index pairs -- m / 2 in round 0, m / 4 behind a bind -- and reads stage log2(pairs) - 10 of hi (a bind at m ==
    // 2048 sums for nobody: stage 0, one valid word)
    auto fill = [&](bool bind) {
        unsigned wg = 0;
        ZcWeights *h_w = (ZcWeights *)(h_desc + live.size());
        for (size_t x = 0; x < live.size(); x++) {
            const Inst &s = t[live[x]];
            SopTab p = describe(live[x]);
            for (unsigned j = 0; bind && j < p.n_tables; j++) p.out[j] = s.work[j];
            p.r_m = bind ? host_to_mont(s.ch) : 0;
            p.first_wg = wg;
            p.slot = (uint32_t)live[x];
            h_desc[x] = p;
            const size_t pairs = bind ? s.len / 4 : s.len / 2;
            const unsigned stage = pairs >= LO_WORDS ? log2_floor(pairs) - ZC_LOG2_LO : 0;
            h_w[x] = ZcWeights{d_weights + s.w_off, d_weights + s.w_off + LO_WORDS + zc::stage_at(stage)};
            wg += (unsigned)product_wgs(s.len);
        }
        return wg;
    };
    const auto d_w = [&] { return (const ZcWeights *)(d_desc + live.size()); };
    const auto desc_bytes = [&] { return live.size() * (sizeof(SopTab) + sizeof(ZcWeights)); };
    // the round's coefficients of the instances in `who` from the published class sums; every transcript steps on a thread of its own
    auto step = [&](const std::vector<size_t> &who) {
        parallel_for(who.size(), [&](size_t x) {
            Inst &s = t[who[x]];
            uint64_t c[SOP_SUMS];
            sop::coefficients(sh[who[x]].D, h_sums + SOP_SUMS * who[x], c);
            s.ch = s.w.step(s.pr, sh[who[x]].D, c);
        });
    };
    if (!live.empty()) {  // round 0: sums over the caller's tables; the copy carries the weights too
        const unsigned wg = fill(false);
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_desc, L.desc_bytes + L.w_bytes, hipMemcpyHostToDevice, ctx->stream));
        const DoneFlag done = done_flag(ctx, 2);
        launch_zc_sums(d_desc, d_w(), (unsigned)live.size(), wg, d_part, ctx->stream);
        launch_sop_finish(d_desc, (unsigned)live.size(), d_part, (uint64_t *)pin, ctx->stream, done);
        HIPCHK(ctx, hipGetLastError());
        CHK(wait_published(ctx, done));
        step(live);
    }
    while (!live.empty()) {  // a later round: bind with the last challenge, sum the next round's terms
        for (size_t i : live)
            if (t[i].pr.st != ZIGZ_OK) return t[i].pr.st;
        const unsigned wg = fill(true);
        const size_t bytes = desc_bytes();
        const ZcWeights *dw = d_w();
        const unsigned n_live = (unsigned)live.size();
        next.clear();
        for (size_t i : live) {
            Inst &s = t[i];
            for (unsigned j = 0; j < sh[i].M; j++) s.cur[j] = s.work[j];
            s.len /= 2;
            if (s.len > HOST_TAIL_MAX) next.push_back(i);
        }
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_desc, bytes, hipMemcpyHostToDevice, ctx->stream));
        launch_zc_bind(d_desc, dw, n_live, wg, d_part, ctx->stream);
        if (!next.empty()) {  // (an instance that is 1024 long now has its next round on the host: nobody reads its sums)
            const DoneFlag done = done_flag(ctx, 2);
            launch_sop_finish(d_desc, n_live, d_part, (uint64_t *)pin, ctx->stream, done);
            HIPCHK(ctx, hipGetLastError());
            CHK(wait_published(ctx, done));
            step(next);
        } else {
            HIPCHK(ctx, hipGetLastError());
        }
        live.swap(next);
    }
    // every instance's current tables in one hand-off
    for (size_t i = 0; i < k; i++) {
        SopTab p = describe(i);
        p.tail_off = t[i].tail_off;
        h_tdesc[i] = p;
    }
    HIPCHK(ctx, hipMemcpyAsync((void *)d_tdesc, h_tdesc, k * sizeof(SopTab), hipMemcpyHostToDevice, ctx->stream));
    const DoneFlag done = done_flag(ctx, 2);
    launch_sop_tails(d_tdesc, (unsigned)k, (uint32_t *)(pin + L.tail_off), ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    const uint32_t *h_tail = (const uint32_t *)(pin + L.tail_off);
    for (size_t x = 0; x < L.tail_words; x++)
        if (h_tail[x] >= P) {  // (a device table is not checked on the way in)
            set_err(ctx, "%s", NOT_CANONICAL_TEXT);
            return ZIGZ_ERR_NOT_CANONICAL;
        }
    parallel_for(k, [&](size_t i) {
        Inst &s = t[i];
        std::vector<uint64_t> f[SOP_MAX_TABLES];
        for (unsigned j = 0; j < sh[i].M; j++) f[j].assign(h_tail + s.tail_off + j * s.len, h_tail + s.tail_off + (j + 1) * s.len);
        const uint64_t c = zc::tail_rounds(s.pr, s.w, f, sh[i].M, sh[i].terms, sh[i].T, sh[i].D, table_evals + sh[i].moff);
        if (s.pr.st != ZIGZ_OK) return;
        eq_evals[i] = pv::eq_at(s.w.tau, s.pr.point, s.w.v, true);
        final_evals[i] = f_mul(eq_evals[i], c);
    });
    for (const Inst &s : t)
        if (s.pr.st != ZIGZ_OK) return s.pr.st;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

zigz_status verify(zigz_ctx *ctx, const zc::VerifyArgs &a, bool host_tables, uint8_t *verdicts, uint64_t *expected_evals,
                   uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    const size_t k = a.k;
    const bool reversed = (a.flags & ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED) != 0;
    const std::vector<sop::Shape> sh = sop::shapes(k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs);
    const std::vector<size_t> roff = zc::round_offsets(sh);
    // one pair of the eval launch per pool table
    std::vector<size_t> pair_ns, owner;
    std::vector<uint64_t> pair_points;
    for (size_t i = 0; i < k; i++)
        for (unsigned j = 0; j < sh[i].M; j++) {
            pair_ns.push_back(a.ns[i]);
            owner.push_back(i);
            pair_points.insert(pair_points.end(), a.points + sh[i].voff, a.points + sh[i].voff + sh[i].nv);
        }
    const size_t m = pair_ns.size();
    DoneFlag done;
    const uint64_t *pairs = nullptr;
    CHK(mle_eval_pairs_queue(ctx, a.tables, host_tables, pair_ns.data(), m, pair_points.data(), reversed, owner.data(), &pairs, &done,
                             bad_index));
    // the k replays and eq(tau, q), underneath the evaluation
    std::vector<sv::Replay> rep(k);
    std::vector<uint64_t> eq(k, 0);
    parallel_for(k, [&](size_t i) {
        rep[i] = pv::replay_rounds(a.claimed_sums[i], a.rounds + roff[i], sh[i].nv, sh[i].D + 1);
        eq[i] = pv::eq_at(a.eq_points + sh[i].voff, a.points + sh[i].voff, sh[i].nv, reversed);
    });
    if (m) CHK(wait_published(ctx, done));
    size_t rejected = 0;
    for (size_t i = 0; i < k; i++) {
        const uint8_t ok = zc::verdict(rep[i], sh[i].terms, sh[i].T, pairs + sh[i].moff, sh[i].M, eq[i], a.final_evals[i],
                                       a.table_evals ? a.table_evals + sh[i].moff : nullptr, a.eq_evals ? a.eq_evals + i : nullptr);
        rejected += !ok;
        if (verdicts) verdicts[i] = ok;
        if (expected_evals) expected_evals[i] = rep[i].expected;
    }
    if (oracle_evals) memcpy(oracle_evals, pairs, m * 8);
    *n_rejected = rejected;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_dev_sumcheck_prove_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables,
                                                               const uint32_t *const *d_tables, const size_t *ns, const unsigned *n_terms,
                                                               const unsigned *term_degrees, const uint8_t *term_tables,
                                                               const uint64_t *term_coeffs, const uint64_t *eq_points,
                                                               const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                               uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals,
                                                               uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const zc::Args a{{k, n_tables, (const void *const *)d_tables, ns, n_terms, term_degrees, term_tables, term_coeffs, fixed_challenges,
                      claimed_sums, rounds, points, table_evals, final_evals},
                     eq_points, eq_evals};
    CHK(zc::check_zerocheck_batch(a, true, false, bad_index));
    return run(ctx, a, d_tables, nullptr, claimed_sums, rounds, points, table_evals, eq_evals, final_evals, bad_index);
}

extern "C" zigz_status zigz_sumcheck_prove_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                           const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                           const uint8_t *term_tables, const uint64_t *term_coeffs,
                                                           const uint64_t *eq_points, const uint64_t *fixed_challenges,
                                                           uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points,
                                                           uint64_t *table_evals, uint64_t *eq_evals, uint64_t *final_evals,
                                                           size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const zc::Args a{{k, n_tables, (const void *const *)tables, ns, n_terms, term_degrees, term_tables, term_coeffs, fixed_challenges,
                      claimed_sums, rounds, points, table_evals, final_evals},
                     eq_points, eq_evals};
    ZIGZ_NOTHROW_BEGIN
    bool value = false;
    const zigz_status st = zc::check_zerocheck_batch_host(a, bad_index, &value);
    if (value) set_err(ctx, "%s", NOT_CANONICAL_TEXT);
    CHK(st);
    ZIGZ_NOTHROW_END(ctx)
    return run(ctx, a, nullptr, tables, claimed_sums, rounds, points, table_evals, eq_evals, final_evals, bad_index);
}

extern "C" zigz_status zigz_dev_sumcheck_verify_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables,
                                                                const uint32_t *const *d_tables, const uint64_t *eq_points,
                                                                const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                                const uint8_t *term_tables, const uint64_t *term_coeffs,
                                                                const uint64_t *claimed_sums, const uint64_t *rounds,
                                                                const uint64_t *points, const uint64_t *table_evals,
                                                                const uint64_t *eq_evals, const uint64_t *final_evals, uint32_t flags,
                                                                uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                                size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const zc::VerifyArgs a{k, n_tables, (const void *const *)d_tables, eq_points, ns, n_terms, term_degrees, term_tables, term_coeffs,
                           claimed_sums, rounds, points, table_evals, eq_evals, final_evals, flags, n_rejected};
    CHK(zc::check_verify_zerocheck_batch(a, true, false, bad_index));
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify(ctx, a, false, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_sumcheck_verify_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                            const uint64_t *eq_points, const size_t *ns, const unsigned *n_terms,
                                                            const unsigned *term_degrees, const uint8_t *term_tables,
                                                            const uint64_t *term_coeffs, const uint64_t *claimed_sums,
                                                            const uint64_t *rounds, const uint64_t *points, const uint64_t *table_evals,
                                                            const uint64_t *eq_evals, const uint64_t *final_evals, uint32_t flags,
                                                            uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                            size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const zc::VerifyArgs a{k, n_tables, (const void *const *)tables, eq_points, ns, n_terms, term_degrees, term_tables, term_coeffs,
                           claimed_sums, rounds, points, table_evals, eq_evals, final_evals, flags, n_rejected};
    bool value = false;
    const zigz_status st = zc::check_verify_zerocheck_batch_host(a, bad_index, &value);
    if (value) set_err(ctx, "%s", NOT_CANONICAL_TEXT);
    CHK(st);
    if (k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    return verify(ctx, a, true, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}
