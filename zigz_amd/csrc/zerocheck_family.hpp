#pragma once
// What the closed-form zero-check hands the round schedule of product_schedule.hpp, shared by its own entries
// (api_zerocheck.cpp) and the grand-product prover, whose layers are instances of it (api_grand_product.cpp).  Its data passes are
// k_zc_sums and k_zc_bind, its finish and tails launches the sop ones; the host turns the class sums into the D + 1 coefficients of
// t_r (sop_host.hpp: coefficients), multiplies by the round's linear factor and the prefix scalar (zerocheck_host.hpp: Weight) and
// steps with D + 2 coefficients.  Behind every descriptor goes the instance's ZcWeights (two pointers), and the FIRST copy also
// carries the weights themselves -- per live instance the 1024 words of lo and the stages of hi, fewer than 2^(v - 10) words
// (zerocheck_host.hpp: build_weights, weight_words) --, which stay where they are for the rest of the call: a round only points
// at its stage (zerocheck_host.hpp: stage).  The tails are finished by zc::tail_rounds; eq(tau, q) is a closed form on the host.
#include "product_schedule.hpp"
#include "zerocheck_host.hpp"

static_assert(sop::MAX_TABLES == SOP_MAX_TABLES && sop::MAX_TERMS == SOP_MAX_TERMS && sop::SUMS == SOP_SUMS, "header, host and kernels");
static_assert(zc::LOG2_LO == ZC_LOG2_LO && pd::R1 == R_MOD_P, "the host builds the weights the way the kernels split and multiply them");
static_assert(sizeof(SopTab) % alignof(ZcWeights) == 0, "the weights' pointers go right behind the descriptors");

namespace sched {

struct ZeroCheck : PoolTerms {
    static constexpr size_t BEHIND = sizeof(ZcWeights);
    static constexpr size_t LO_WORDS = (size_t)1 << ZC_LOG2_LO;
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

}  // namespace sched
