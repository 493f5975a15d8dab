#pragma once
// The host side of the batched product sumcheck prover (api_product.cpp, sumcheck_product.hip): the argument
// checks of the two entries, the round coefficients from the sums the kernels publish, the rounds of a table that has become
// small enough for the host, and one instance's transcript (SumcheckProver.prove, src/proofs/sumcheck_prover.zig:26-91, with
// d + 1 coefficients per round: generateChallenge absorbs however many a round has, sumcheck_protocol.zig:176-184).  Plain
// C++, no HIP: the header is testable without a GPU (tests/c_driver/product_host.cpp), like sumcheck_verify_host.hpp.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "batch_host.hpp"  // canonical(), checks_in_call_order()
#include "host_hash.hpp"
#include "sumcheck_verify_host.hpp"  // the field helpers and Multilinear.init's shape rule
#include "zigz_hip.h"

namespace zk {
namespace pd {

using sv::bad_at;
using sv::f_add;
using sv::f_mul;
using sv::log2_of;

constexpr uint64_t PD_P = ZIGZ_BABYBEAR_P;
constexpr unsigned MAX_DEGREE = ZIGZ_PRODUCT_MAX_DEGREE;
constexpr size_t TAIL_MAX = 1024;  // a table this long or shorter finishes its rounds on the host (k_batch_tails' threshold)

inline uint64_t f_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + PD_P - b; }

// What zigz_[dev_]sumcheck_prove_product_batch says about its arguments before anything runs: ZIGZ_OK, or the status of the
// first instance it rejects, whose index goes to *bad_index.  factors: sum d_i pointers, instance by instance.  dev: device
// pointers (16-byte aligned, never read here); otherwise host tables, whose values are checked when `values` is set (the
// library checks them while it narrows them instead).  *first_factor (may be NULL): the rejected instance's first entry in
// `factors`.  k == 0 is ZIGZ_OK.
inline zigz_status check_product_batch(size_t k, const unsigned *degrees, const void *const *factors, const size_t *ns,
                                       const uint64_t *fixed, const void *claimed_sums, const void *rounds, const void *points,
                                       const void *factor_evals, const void *final_evals, bool dev, bool values, size_t *bad_index,
                                       size_t *first_factor = nullptr) {
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !degrees || !factors || !ns || !claimed_sums || !rounds || !points || !factor_evals || !final_evals)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    size_t foff = 0, voff = 0;
    for (size_t i = 0; i < k; i++) {
        if (first_factor) *first_factor = foff;
        const unsigned d = degrees[i];
        if (d < 1 || d > MAX_DEGREE) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const void *const *f = factors + foff;
        if (dev)
            for (unsigned j = 0; j < d; j++)
                if (!f[j]) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const zigz_status st = sv::shape(ns[i]);
        if (st != ZIGZ_OK) return bad_at(bad_index, i, st);
        const size_t v = log2_of(ns[i]);
        if (v > ZIGZ_PRODUCT_MAX_LOG2_N) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        if (ns[i] == 1) return bad_at(bad_index, i, ZIGZ_ERR_NO_VARIABLES);
        for (unsigned j = 0; j < d; j++)
            if (!f[j] || (dev && ((uintptr_t)f[j] & 15))) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        if (!dev && values)
            for (unsigned j = 0; j < d; j++)
                if (!canonical((const uint64_t *)f[j], ns[i])) return bad_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        if (fixed && !canonical(fixed + voff, v)) return bad_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        foff += d;
        voff += v;
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
constexpr uint64_t R1 = ((uint64_t)1 << 32) % PD_P;
constexpr uint64_t R2 = (R1 * R1) % PD_P;
constexpr uint64_t R3 = (R2 * R1) % PD_P;
static_assert(MAX_DEGREE == 3, "one scale per degree");
inline uint64_t sum_scale(unsigned d) { return d == 1 ? 1 : d == 2 ? R2 : R3; }

// the d + 1 canonical coefficients of a round from the d + 1 sums (each below p) the finish launch wrote
inline void coefficients(unsigned d, const uint64_t *sums, uint64_t *c) {
    const uint64_t s = sum_scale(d);
    for (unsigned j = 0; j <= d; j++) c[j] = f_mul(sums[j], s);
}

// the same coefficients from the tables themselves (m >= 2 canonical values per factor): g(t) = sum_{i < m/2} prod_j (a_j + t
// (b_j - a_j)) with a_j = f_j[i], b_j = f_j[i + m/2]
inline void round_coefficients(unsigned d, const std::vector<uint64_t> *f, size_t m, uint64_t *c) {
    const size_t half = m / 2;
    for (unsigned j = 0; j <= d; j++) c[j] = 0;
    for (size_t i = 0; i < half; i++) {
        uint64_t g[MAX_DEGREE + 1] = {1, 0, 0, 0};
        for (unsigned j = 0; j < d; j++) {  // g *= a + e t
            const uint64_t a = f[j][i], e = f_sub(f[j][i + half], a);
            for (unsigned x = j + 1; x > 0; x--) g[x] = f_add(f_mul(g[x], a), f_mul(g[x - 1], e));
            g[0] = f_mul(g[0], a);
        }
        for (unsigned j = 0; j <= d; j++) c[j] = f_add(c[j], g[j]);
    }
}

// One instance's prover: its transcript, round counter and outputs.
struct Prover {
    unsigned d = 0;
    size_t nv = 0, round = 0;
    uint64_t *claimed_sum = nullptr, *rounds = nullptr, *point = nullptr;
    const uint64_t *fixed = nullptr;  // caller-fixed challenges (checked canonical), or none: drawn from the transcript
    Transcript tr;                    // fresh per instance, sumcheck_protocol.zig:161
    zigz_status st = ZIGZ_OK;

    // generateChallenge (sumcheck_protocol.zig:176-184): records the round polynomial c_0..c_d -- the first round's g(0) + g(1)
    // is the claimed sum --, then takes the fixed challenge or absorbs the coefficients in order and draws one
    uint64_t challenge(const uint64_t *c) {
        if (round == 0) {
            uint64_t s = c[0];
            for (unsigned j = 0; j <= d; j++) s = f_add(s, c[j]);
            *claimed_sum = s;
        }
        for (unsigned j = 0; j <= d; j++) rounds[(d + 1) * round + j] = c[j];
        uint64_t ch;
        if (fixed) {
            ch = fixed[round];
        } else {
            for (unsigned j = 0; j <= d; j++) tr.append_field(c[j]);
            ch = tr.challenge();
        }
        point[round++] = ch;
        return ch;
    }
    // the last rounds on the remaining tables (f[j]: m <= TAIL_MAX values each; bound in place, MSB-first like partialEval,
    // multilinear.zig:166-173); writes every factor fully bound and returns their product, final_eval
    uint64_t tail_rounds(std::vector<uint64_t> *f, uint64_t *factor_evals) {
        size_t m = f[0].size();
        while (m > 1) {
            uint64_t c[MAX_DEGREE + 1];
            round_coefficients(d, f, m, c);
            const uint64_t ch = challenge(c);
            const size_t half = m / 2;
            for (unsigned j = 0; j < d; j++) {
                for (size_t x = 0; x < half; x++) f[j][x] = f_add(f[j][x], f_mul(ch, f_sub(f[j][x + half], f[j][x])));
                f[j].resize(half);
            }
            m = half;
        }
        if (round != nv) st = ZIGZ_ERR_PROTOCOL_ERROR;  // sumcheck_prover.zig:80-82
        uint64_t fe = 1;
        for (unsigned j = 0; j < d; j++) {
            factor_evals[j] = f[j][0];
            fe = f_mul(fe, f[j][0]);
        }
        return fe;
    }
};

}  // namespace pd
}  // namespace zk
