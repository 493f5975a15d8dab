#pragma once
// The host side of the batched product sumcheck prover (api_product.cpp, sumcheck_product.hip) that is its own:
// the argument checks of the two entries and the round coefficients from the sums the kernels publish.  An instance's transcript,
// round step and host rounds are sumcheck_host.hpp's (SumcheckRounds with d + 1 coefficients per round: generateChallenge absorbs
// however many a round has, sumcheck_protocol.zig:176-184).  Plain C++, no HIP: the header is testable without a GPU
// (tests/c_driver/product_host.cpp), like sumcheck_verify_host.hpp.
#include "sumcheck_host.hpp"

namespace zk {
namespace pd {

constexpr unsigned MAX_DEGREE = SUMCHECK_MAX_DEGREE;

// What zigz_[dev_]sumcheck_prove_product_batch says about its arguments before anything runs: ZIGZ_OK, or the status of the
// first instance it rejects, whose index goes to *bad_index (sumcheck_host.hpp: table_rule; dev, values as there).  factors: sum
// d_i pointers, instance by instance.  *first_factor (may be NULL): the rejected instance's first entry in `factors`.  k == 0 is
// ZIGZ_OK.
inline zigz_status check_product_batch(size_t k, const unsigned *degrees, const void *const *factors, const size_t *ns,
                                       const uint64_t *fixed, const void *claimed_sums, const void *rounds, const void *points,
                                       const void *factor_evals, const void *final_evals, bool dev, bool values, size_t *bad_index,
                                       size_t *first_factor = nullptr) {
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !degrees || !factors || !ns || !claimed_sums || !rounds || !points || !factor_evals || !final_evals)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, values, true, false, ZIGZ_PRODUCT_MAX_LOG2_N};
    size_t foff = 0, voff = 0;
    for (size_t i = 0; i < k; i++) {
        if (first_factor) *first_factor = foff;
        const unsigned d = degrees[i];
        if (d < 1 || d > MAX_DEGREE) return fail_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const zigz_status st = table_rule(rule, factors + foff, d, ns[i], fixed ? fixed + voff : nullptr);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        foff += d;
        voff += log2_floor(ns[i]);
    }
    return ZIGZ_OK;
}

// The host form's checks in the family's order (batch_host.hpp: checks_in_call_order, over the factors one behind the other):
// a factor holding a value >= p BEFORE the first instance that fails another check is reported instead, with its instance.
inline zigz_status check_product_batch_host(size_t k, const unsigned *degrees, const uint64_t *const *factors, const size_t *ns,
                                            const uint64_t *fixed, const void *claimed_sums, const void *rounds, const void *points,
                                            const void *factor_evals, const void *final_evals, size_t *bad_index,
                                            bool *value_found = nullptr) {
    size_t bad = k, ff = 0;
    const zigz_status st = check_product_batch(k, degrees, (const void *const *)factors, ns, fixed, claimed_sums, rounds, points,
                                               factor_evals, final_evals, false, false, &bad, &ff);
    if (value_found) *value_found = false;
    if (st == ZIGZ_OK || bad >= k) return st;
    // the factors in front of the failing instance (their degrees and pointers have passed), and which instance each belongs to
    std::vector<size_t> fns, owner;
    for (size_t i = 0; i < bad; i++)
        for (unsigned j = 0; j < degrees[i]; j++) {
            fns.push_back(ns[i]);
            owner.push_back(i);
        }
    size_t fbad = ff;
    const zigz_status st2 = checks_in_call_order(factors, fns.data(), ff + 1, &fbad, [&](size_t *f) {
        *f = ff;
        return st;
    }, value_found);
    if (bad_index) *bad_index = fbad < ff ? owner[fbad] : bad;
    return st2;
}

// R^d mod p for the sums of a degree-d instance: the kernels publish a coefficient of d >= 2 factors times R^-d (the factor
// 1/R a Montgomery product of two canonical values carries is not repaired per element; sumcheck_product.hip)
constexpr uint64_t R1 = ((uint64_t)1 << 32) % ZIGZ_BABYBEAR_P;
constexpr uint64_t R2 = (R1 * R1) % ZIGZ_BABYBEAR_P;
constexpr uint64_t R3 = (R2 * R1) % ZIGZ_BABYBEAR_P;
static_assert(MAX_DEGREE == 3, "one scale per degree");
inline uint64_t sum_scale(unsigned d) { return d == 1 ? 1 : d == 2 ? R2 : R3; }

// the d + 1 canonical coefficients of a round from the d + 1 sums (each below p) the finish launch wrote
inline void coefficients(unsigned d, const uint64_t *sums, uint64_t *c) {
    const uint64_t s = sum_scale(d);
    for (unsigned j = 0; j <= d; j++) c[j] = f_mul(sums[j], s);
}

}  // namespace pd
}  // namespace zk
