// C ABI of libzigz_hip.so, part 9: the batched product sumcheck prover.  The schedule is product_schedule.hpp's;
// here: what the product family hands it -- d factor tables per instance, d + 1 sums and coefficients per round
// (product_host.hpp), the host rounds of sumcheck_host.hpp -- and the two entries.
#include "product_schedule.hpp"
#include "product_host.hpp"

using namespace zk;

static_assert(pd::MAX_DEGREE == PRODUCT_MAX_DEGREE && ZIGZ_PRODUCT_MAX_LOG2_N == PRODUCT_MAX_LOG2_N, "header, host and kernels");
static_assert(pd::R1 == R_MOD_P && pd::R2 == R2_MOD_P, "the host's scales are powers of the kernels' R");

namespace {

struct Product {
    using Tab = ProductTab;
    static constexpr unsigned SUMS = PRODUCT_SUMS, MAX_TABLES = PRODUCT_MAX_DEGREE;
    static constexpr size_t BEHIND = 0;
    const unsigned *degrees;
    uint64_t *factor_evals, *final_evals;
    std::vector<size_t> feoff;  // instance i's first factor

    Product(size_t k, const unsigned *degrees, uint64_t *factor_evals, uint64_t *final_evals)
        : degrees(degrees), factor_evals(factor_evals), final_evals(final_evals), feoff(k + 1, 0) {
        for (size_t i = 0; i < k; i++) feoff[i + 1] = feoff[i] + degrees[i];
    }
    unsigned n_tables(size_t i) const { return degrees[i]; }
    unsigned ncoef(size_t i) const { return degrees[i] + 1; }
    void describe(size_t i, ProductTab &p) const { p.d = degrees[i]; }
    size_t payload_words(size_t) const { return 0; }
    void payload(size_t, uint32_t *) const {}
    void behind(size_t, void *, const uint32_t *, size_t, bool) const {}
    void sums(const ProductTab *d, unsigned n, unsigned wg, unsigned long long *part, hipStream_t s) const {
        launch_product_sums(d, n, wg, part, s);
    }
    void bind(const ProductTab *d, unsigned n, unsigned wg, unsigned long long *part, hipStream_t s) const {
        launch_product_bind(d, n, wg, part, s);
    }
    void finish(const ProductTab *d, unsigned n, const unsigned long long *part, uint64_t *out, hipStream_t s, DoneFlag done) const {
        launch_product_finish(d, n, part, out, s, done);
    }
    void tails(const ProductTab *d, unsigned n, uint32_t *h_dst, hipStream_t s, DoneFlag done) const {
        launch_product_tails(d, n, h_dst, s, done);
    }
    uint64_t step(size_t i, SumcheckRounds &pr, const uint64_t *sums) const {
        uint64_t c[PRODUCT_SUMS];
        pd::coefficients(degrees[i], sums, c);
        return pr.step(c);
    }
    void finish_tail(size_t i, SumcheckRounds &pr, std::vector<uint64_t> *f) const {
        final_evals[i] = pr.tail_rounds(f, factor_evals + feoff[i]);
    }
};

zigz_status run(zigz_ctx *ctx, size_t k, const unsigned *degrees, const uint32_t *const *d_factors, const uint64_t *const *h_factors,
                const size_t *ns, const uint64_t *fixed, uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points,
                uint64_t *factor_evals, uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    Product fam(k, degrees, factor_evals, final_evals);
    return sched::run(ctx, fam, k, d_factors, h_factors, ns, fixed, claimed_sums, rounds, points, bad_index);
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
    CHK(host_value_checks(ctx, [&](bool *value) {
        return pd::check_product_batch_host(k, degrees, factors, ns, fixed_challenges, claimed_sums, rounds, points, factor_evals,
                                            final_evals, bad_index, value);
    }));
    ZIGZ_NOTHROW_END(ctx)
    return run(ctx, k, degrees, nullptr, factors, ns, fixed_challenges, claimed_sums, rounds, points, factor_evals, final_evals,
               bad_index);
}
