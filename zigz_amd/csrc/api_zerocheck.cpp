// C ABI of libzigz_hip.so, part 11: the zero-check sumcheck with the eq factor in closed form and its verifier.
// The schedule and the verifier are product_schedule.hpp's, over a pool WITHOUT eq; here: what the zero-check family hands them.
// Its data passes are k_zc_sums and k_zc_bind, its finish and tails launches the sop ones; the host turns the class sums into the
// D + 1 coefficients of t_r (sop_host.hpp: coefficients), multiplies by the round's linear factor and the prefix scalar
// (zerocheck_host.hpp: Weight) and steps with D + 2 coefficients.  Behind every descriptor goes the instance's ZcWeights (two
// pointers), and the FIRST copy also carries the weights themselves -- per live instance the 1024 words of lo and the stages of
// hi, fewer than 2^(v - 10) words (zerocheck_host.hpp: build_weights, weight_words) --, which stay where they are for the rest of
// the call: a round only points at its stage (zerocheck_host.hpp: stage).  The tails are finished by zc::tail_rounds; eq(tau, q)
// is a closed form on the host, for the prover and the verifier.
#include "product_schedule.hpp"
#include "zerocheck_host.hpp"

using namespace zk;

static_assert(sop::MAX_TABLES == SOP_MAX_TABLES && sop::MAX_TERMS == SOP_MAX_TERMS && sop::SUMS == SOP_SUMS, "header, host and kernels");
static_assert(zc::LOG2_LO == ZC_LOG2_LO && pd::R1 == R_MOD_P, "the host builds the weights the way the kernels split and multiply them");
static_assert(sizeof(SopTab) % alignof(ZcWeights) == 0, "the weights' pointers go right behind the descriptors");

namespace {

constexpr size_t LO_WORDS = (size_t)1 << ZC_LOG2_LO;

struct ZeroCheck : sched::PoolTerms {
    static constexpr size_t BEHIND = sizeof(ZcWeights);
    uint64_t *table_evals, *eq_evals, *final_evals;
    struct alignas(64) Own : zc::Weight {};  // a cache line of its own: every step moves P on, on a thread of the instance's own
    std::vector<Own> w;

    ZeroCheck(const zc::Args &za, uint64_t *table_evals, uint64_t *eq_evals, uint64_t *final_evals)
        : PoolTerms(za.s), table_evals(table_evals), eq_evals(eq_evals), final_evals(final_evals), w(za.s.k) {
        for (size_t i = 0; i < za.s.k; i++) {
            w[i].tau = za.eq_points + sh[i].voff;
            w[i].v = sh[i].nv;
        }
    }
    unsigned ncoef(size_t i) const { return sh[i].D + 2; }
    size_t payload_words(size_t n) const { return zc::weight_words(n); }
    void payload(size_t i, uint32_t *h) const { zc::build_weights(w[i].tau, (unsigned)w[i].v, ZC_LOG2_LO, h, h + LO_WORDS); }
    void behind(size_t, void *h, const uint32_t *d_weights, size_t m, bool bind) const {
        *(ZcWeights *)h = ZcWeights{d_weights, d_weights + LO_WORDS + zc::stage_at(zc::stage(m, bind))};
    }
    void sums(const SopTab *d, unsigned n, unsigned wg, unsigned long long *part, hipStream_t s) const {
        launch_zc_sums(d, (const ZcWeights *)(d + n), n, wg, part, s);
    }
    void bind(const SopTab *d, unsigned n, unsigned wg, unsigned long long *part, hipStream_t s) const {
        launch_zc_bind(d, (const ZcWeights *)(d + n), n, wg, part, s);
    }
    uint64_t step(size_t i, SumcheckRounds &pr, const uint64_t *sums) {
        uint64_t c[SOP_SUMS];
        sop::coefficients(sh[i].D, sums, c);
        return w[i].step(pr, sh[i].D, c);
    }
    void finish_tail(size_t i, SumcheckRounds &pr, std::vector<uint64_t> *f) {
        const uint64_t c = zc::tail_rounds(pr, w[i], f, sh[i].M, sh[i].terms, sh[i].T, sh[i].D, table_evals + sh[i].moff);
        if (pr.st != ZIGZ_OK) return;
        eq_evals[i] = pv::eq_at(w[i].tau, pr.point, w[i].v, true);
        final_evals[i] = f_mul(eq_evals[i], c);
    }
};

zigz_status run(zigz_ctx *ctx, const zc::Args &za, const uint32_t *const *d_tables, const uint64_t *const *h_tables,
                uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals,
                uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    ZeroCheck fam(za, table_evals, eq_evals, final_evals);
    return sched::run(ctx, fam, za.s.k, d_tables, h_tables, za.s.ns, za.s.fixed, claimed_sums, rounds, points, bad_index);
    ZIGZ_NOTHROW_END(ctx)
}

// the verifier's entry: every pool entry is a table; eq(tau, q) is one closed form per proof
struct ZcVerify {
    const zc::VerifyArgs &a;
    const std::vector<sop::Shape> &sh;
    const std::vector<size_t> roffs;
    std::vector<uint64_t> eq;

    ZcVerify(const zc::VerifyArgs &a, const std::vector<sop::Shape> &sh) : a(a), sh(sh), roffs(zc::round_offsets(sh)), eq(a.k, 0) {}
    bool is_pair(size_t) const { return true; }
    unsigned degree(size_t i) const { return sh[i].D + 1; }
    size_t roff(size_t i) const { return roffs[i]; }
    void host_values(size_t i, bool reversed, uint64_t *) {
        eq[i] = pv::eq_at(a.eq_points + sh[i].voff, a.points + sh[i].voff, sh[i].nv, reversed);
    }
    uint8_t verdict(size_t i, const sv::Replay &rep, const uint64_t *ev) const {
        return zc::verdict(rep, sh[i].terms, sh[i].T, ev, sh[i].M, eq[i], a.final_evals[i],
                           a.table_evals ? a.table_evals + sh[i].moff : nullptr, a.eq_evals ? a.eq_evals + i : nullptr);
    }
};

zigz_status verify(zigz_ctx *ctx, const zc::VerifyArgs &a, bool host_tables, uint8_t *verdicts, uint64_t *expected_evals,
                   uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    if (a.k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    ZIGZ_NOTHROW_BEGIN
    const std::vector<sop::Shape> sh = sop::shapes(a.k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs);
    ZcVerify entry(a, sh);
    return sched::verify_pool(ctx, a, sh, entry, host_tables, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
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
    CHK(host_value_checks(ctx, [&](bool *value) { return zc::check_zerocheck_batch_host(a, bad_index, value); }));
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
    CHK(host_value_checks(ctx, [&](bool *value) { return zc::check_verify_zerocheck_batch_host(a, bad_index, value); }));
    return verify(ctx, a, true, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}
