// C ABI of libzigz_hip.so, part 9: the batched product sumcheck prover.
//
// Schedule of one call.  Instances longer than 1024 are LIVE.  Round 0: the host writes the live instances' descriptors into
// pinned memory and queues one copy of them, one launch that sums every live instance's round-0 terms over the caller's tables
// and one small launch that reduces them into pinned memory and stores the completion word; the host polls that word, turns
// the sums into coefficients and steps every live transcript on its threads.  Every later round is the same copy and two
// launches with the fused bind pass in place of the sums (the first one writes each factor's bound copy, n/2 words, into the
// workspace; the later ones run in place there); an instance leaves the live set when its tables are 1024 long.  One launch
// then hands the current tables of ALL instances to the host, which finishes their rounds (sumcheck_host.hpp).
#include "api_internal.hpp"
#include "product_host.hpp"

using namespace zk;

static_assert(pd::MAX_DEGREE == PRODUCT_MAX_DEGREE && ZIGZ_PRODUCT_MAX_LOG2_N == PRODUCT_MAX_LOG2_N, "header, host and kernels");
static_assert(pd::R1 == R_MOD_P && pd::R2 == R2_MOD_P, "the host's scales are powers of the kernels' R");

namespace {

struct Inst {
    unsigned d = 0;
    size_t len = 0, tail_off = 0;
    const uint32_t *cur[PRODUCT_MAX_DEGREE] = {};
    uint32_t *work[PRODUCT_MAX_DEGREE] = {};
    uint64_t ch = 0;  // the challenge of the instance's last round
    SumcheckRounds pr;
};

// one call's pinned region: sums (PRODUCT_SUMS u64 per instance) | tails (u32) | round descriptors | tail descriptors | the
// narrowed tables of the host form
struct Layout {
    size_t tail_off = 0, tail_words = 0, desc_off = 0, tdesc_off = 0, tab_off = 0, tab_words = 0, bytes = 0;
    size_t nwg = 0, work_words = 0;  // workgroups of round 0; words of all bound copies
    std::vector<size_t> fns, owner;  // every factor's length and instance
    std::vector<size_t> at;          // host form: factor f's first word among the narrowed tables (each 16-byte aligned)
};

zigz_status plan(size_t k, const unsigned *degrees, const size_t *ns, bool host_tables, Layout &L) {
    for (size_t i = 0; i < k; i++) {
        L.tail_words += degrees[i] * (ns[i] < HOST_TAIL_MAX ? ns[i] : HOST_TAIL_MAX);
        if (ns[i] > HOST_TAIL_MAX) {
            L.nwg += product_wgs(ns[i]);
            L.work_words += degrees[i] * (ns[i] / 2);
        }
        L.fns.insert(L.fns.end(), degrees[i], ns[i]);
        L.owner.insert(L.owner.end(), degrees[i], i);
    }
    if (L.nwg > MLE_BATCH_MAX_WGS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    const size_t desc = align256(k * sizeof(ProductTab));
    L.tail_off = align256(k * PRODUCT_SUMS * 8);
    L.desc_off = L.tail_off + align256(L.tail_words * 4);
    L.tdesc_off = L.desc_off + desc;
    L.tab_off = L.tdesc_off + desc;
    if (host_tables) {
        L.at = packed_offsets(L.fns.data(), L.fns.size());
        L.tab_words = L.at[L.fns.size()];
    }
    L.bytes = L.tab_off + L.tab_words * 4;
    return ZIGZ_OK;
}

zigz_status run(zigz_ctx *ctx, size_t k, const unsigned *degrees, const uint32_t *const *d_factors, const uint64_t *const *h_factors,
                const size_t *ns, const uint64_t *fixed, uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points,
                uint64_t *factor_evals, uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    Layout L;
    CHK(plan(k, degrees, ns, h_factors != nullptr, L));
    uint8_t *pin;
    CHK(pinned(ctx, L.bytes, &pin));
    std::vector<const uint32_t *> up;
    if (h_factors) {
        CHK(stage_host_tables(ctx, h_factors, L.fns.data(), L.fns.size(), L.at, (uint32_t *)(pin + L.tab_off), WS_PRODUCT_IN,
                              L.owner.data(), up, bad_index));
        d_factors = up.data();
    }
    const size_t desc = L.tdesc_off - L.desc_off;
    void *d_stage, *d_work;
    CHK(ws_get(ctx, WS_PRODUCT, 2 * desc + L.nwg * PRODUCT_SUMS * 8, &d_stage));
    CHK(ws_get(ctx, WS_PRODUCT_WORK, L.work_words * 4, &d_work));
    const ProductTab *d_desc = (const ProductTab *)d_stage, *d_tdesc = (const ProductTab *)((uint8_t *)d_stage + desc);
    unsigned long long *d_part = (unsigned long long *)((uint8_t *)d_stage + 2 * desc);
    ProductTab *h_desc = (ProductTab *)(pin + L.desc_off), *h_tdesc = (ProductTab *)(pin + L.tdesc_off);
    const uint64_t *h_sums = (const uint64_t *)pin;

    std::vector<Inst> t(k);
    std::vector<size_t> live, next;
    {
        size_t foff = 0, voff = 0, roff = 0, woff = 0, toff = 0;
        for (size_t i = 0; i < k; i++) {
            Inst &s = t[i];
            s.d = degrees[i];
            s.len = ns[i];
            s.tail_off = toff;
            toff += s.d * (ns[i] < HOST_TAIL_MAX ? ns[i] : HOST_TAIL_MAX);
            for (unsigned j = 0; j < s.d; j++) {
                s.cur[j] = d_factors[foff + j];
                if (ns[i] > HOST_TAIL_MAX) {  // every factor's bound copy is 16-byte aligned: n / 2 >= 1024 words
                    s.work[j] = (uint32_t *)d_work + woff;
                    woff += ns[i] / 2;
                }
            }
            s.pr.ncoef = s.d + 1;
            s.pr.nv = log2_floor(ns[i]);
            s.pr.claimed_sum = claimed_sums + i;
            s.pr.rounds = rounds + roff;
            s.pr.point = points + voff;
            s.pr.fixed = fixed ? fixed + voff : nullptr;
            foff += s.d;
            voff += s.pr.nv;
            roff += (size_t)(s.d + 1) * s.pr.nv;
            if (ns[i] > HOST_TAIL_MAX) live.push_back(i);
        }
    }
    // the live instances' descriptors for one pass; returns its workgroup count
    auto fill = [&](bool bind) {
        unsigned wg = 0;
        for (size_t x = 0; x < live.size(); x++) {
            const Inst &s = t[live[x]];
            ProductTab p{};
            for (unsigned j = 0; j < s.d; j++) {
                p.in[j] = s.cur[j];
                p.out[j] = bind ? s.work[j] : nullptr;
            }
            p.m = s.len;
            p.d = s.d;
            p.r_m = bind ? host_to_mont(s.ch) : 0;
            p.first_wg = wg;
            p.slot = (uint32_t)live[x];
            h_desc[x] = p;
            wg += (unsigned)product_wgs(s.len);
        }
        return wg;
    };
    // the round's coefficients of the instances in `who` from the published sums; every transcript steps on a thread of its own
    auto step = [&](const std::vector<size_t> &who) {
        parallel_for(who.size(), [&](size_t x) {
            Inst &s = t[who[x]];
            uint64_t c[PRODUCT_SUMS];
            pd::coefficients(s.d, h_sums + PRODUCT_SUMS * who[x], c);
            s.ch = s.pr.step(c);
        });
    };
    if (!live.empty()) {  // round 0: sums over the caller's tables
        const unsigned wg = fill(false);
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_desc, live.size() * sizeof(ProductTab), hipMemcpyHostToDevice, ctx->stream));
        const DoneFlag done = done_flag(ctx, 2);
        launch_product_sums(d_desc, (unsigned)live.size(), wg, d_part, ctx->stream);
        launch_product_finish(d_desc, (unsigned)live.size(), d_part, (uint64_t *)pin, ctx->stream, done);
        HIPCHK(ctx, hipGetLastError());
        CHK(wait_published(ctx, done));
        step(live);
    }
    while (!live.empty()) {  // a later round: bind with the last challenge, sum the next round's terms
        const unsigned wg = fill(true);
        next.clear();
        for (size_t i : live) {
            Inst &s = t[i];
            for (unsigned j = 0; j < s.d; j++) s.cur[j] = s.work[j];
            s.len /= 2;
            if (s.len > HOST_TAIL_MAX) next.push_back(i);
        }
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_desc, live.size() * sizeof(ProductTab), hipMemcpyHostToDevice, ctx->stream));
        launch_product_bind(d_desc, (unsigned)live.size(), wg, d_part, ctx->stream);
        if (!next.empty()) {  // (an instance that is 1024 long now has its next round on the host: nobody reads its sums)
            const DoneFlag done = done_flag(ctx, 2);
            launch_product_finish(d_desc, (unsigned)live.size(), d_part, (uint64_t *)pin, ctx->stream, done);
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
        const Inst &s = t[i];
        ProductTab p{};
        for (unsigned j = 0; j < s.d; j++) p.in[j] = s.cur[j];
        p.m = s.len;
        p.d = s.d;
        p.tail_off = s.tail_off;
        h_tdesc[i] = p;
    }
    HIPCHK(ctx, hipMemcpyAsync((void *)d_tdesc, h_tdesc, k * sizeof(ProductTab), hipMemcpyHostToDevice, ctx->stream));
    const DoneFlag done = done_flag(ctx, 2);
    launch_product_tails(d_tdesc, (unsigned)k, (uint32_t *)(pin + L.tail_off), ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    const uint32_t *h_tail = (const uint32_t *)(pin + L.tail_off);
    for (size_t x = 0; x < L.tail_words; x++)
        if (h_tail[x] >= P) {  // (a device table is not checked on the way in)
            set_err(ctx, "%s", NOT_CANONICAL_TEXT);
            return ZIGZ_ERR_NOT_CANONICAL;
        }
    std::vector<size_t> feoff(k + 1, 0);
    for (size_t i = 0; i < k; i++) feoff[i + 1] = feoff[i] + t[i].d;
    parallel_for(k, [&](size_t i) {
        Inst &s = t[i];
        std::vector<uint64_t> f[PRODUCT_MAX_DEGREE];
        for (unsigned j = 0; j < s.d; j++) f[j].assign(h_tail + s.tail_off + j * s.len, h_tail + s.tail_off + (j + 1) * s.len);
        final_evals[i] = s.pr.tail_rounds(f, factor_evals + feoff[i]);
    });
    for (const Inst &s : t)
        if (s.pr.st != ZIGZ_OK) return s.pr.st;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_dev_sumcheck_prove_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                                             const uint32_t *const *d_factors, const size_t *ns,
                                                             const uint64_t *fixed_challenges, uint64_t *claimed_sums,
                                                             uint64_t *rounds, uint64_t *points, uint64_t *factor_evals,
                                                             uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    CHK(pd::check_product_batch(k, degrees, (const void *const *)d_factors, ns, fixed_challenges, claimed_sums, rounds, points,
                                factor_evals, final_evals, true, false, bad_index));
    return run(ctx, k, degrees, d_factors, nullptr, ns, fixed_challenges, claimed_sums, rounds, points, factor_evals, final_evals,
               bad_index);
}

extern "C" zigz_status zigz_sumcheck_prove_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                                         const uint64_t *const *factors, const size_t *ns,
                                                         const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                         uint64_t *points, uint64_t *factor_evals, uint64_t *final_evals,
                                                         size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    ZIGZ_NOTHROW_BEGIN
    bool value = false;
    const zigz_status st = pd::check_product_batch_host(k, degrees, factors, ns, fixed_challenges, claimed_sums, rounds, points,
                                                        factor_evals, final_evals, bad_index, &value);
    if (value) set_err(ctx, "%s", NOT_CANONICAL_TEXT);
    CHK(st);
    ZIGZ_NOTHROW_END(ctx)
    return run(ctx, k, degrees, nullptr, factors, ns, fixed_challenges, claimed_sums, rounds, points, factor_evals, final_evals,
               bad_index);
}
