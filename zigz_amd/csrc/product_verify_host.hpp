#pragma once
// The host side of the batched eq tables and the batched product-proof verification (api_mle_batch.cpp, eq_batch.hip; DESIGN.md
// s7h): the argument checks of the four entries, the replay of a proof's rounds with d + 1 coefficients per round
// (SumcheckVerifier.verify / verifyRounds, src/proofs/sumcheck_verifier.zig:48-108,172-205), eq(tau, .) at a point in closed
// form, and the verdict.  On top of sumcheck_host.hpp (field, table_rule, transcript step) and sumcheck_verify_host.hpp (the
// linear verifier's Replay, which the d = 1 case reproduces word for word).  Plain C++, no HIP: testable without a GPU
// (tests/c_driver/product_verify_host.cpp).
#include "sumcheck_verify_host.hpp"

namespace zk {
namespace pv {

constexpr unsigned MAX_DEGREE = SUMCHECK_MAX_DEGREE;
constexpr uint8_t KIND_TABLE = ZIGZ_FACTOR_TABLE, KIND_EQ = ZIGZ_FACTOR_EQ;

// What zigz_[dev_]eq_table_batch says about its arguments before anything runs: ZIGZ_OK, or the status of the first table it
// rejects, whose index goes to *bad_index (sumcheck_host.hpp: table_rule -- the shape, the length, the output pointer, the
// point's words, in the family's order).  dev: device outputs (16-byte aligned); otherwise host arrays.  k == 0 is ZIGZ_OK.
inline zigz_status check_eq_table_batch(size_t k, const size_t *ns, const uint64_t *points, const void *const *out, bool dev,
                                        size_t *bad_index) {
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !ns || !points || !out) return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, false, false, true, sv::SV_MAX_LOG2_N};
    for (size_t i = 0, off = 0; i < k; off += log2_floor(ns[i++])) {
        const zigz_status st = table_rule(rule, out + i, 1, ns[i], points + off);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
    }
    return ZIGZ_OK;
}

// The arguments of zigz_[dev_]sumcheck_verify_product_batch, as the entries take them (factors: sum d_i pointers, NULL where
// the factor is eq(tau, .); factor_kinds and factor_evals may be NULL)
struct VerifyArgs {
    size_t k;
    const unsigned *degrees;
    const void *const *factors;
    const uint8_t *factor_kinds;
    const uint64_t *eq_points;
    const size_t *ns;
    const uint64_t *claimed_sums, *rounds, *points, *factor_evals, *final_evals;
    uint32_t flags;
    const size_t *n_rejected;
};
inline uint8_t kind_of(const VerifyArgs &a, size_t factor) { return a.factor_kinds ? a.factor_kinds[factor] : KIND_TABLE; }

// What the entries say about their arguments before anything runs: ZIGZ_OK, or the status of the first proof they reject, whose
// index goes to *bad_index.  Per proof, in order: the degree; the kinds (an unknown kind, an eq factor with a table pointer, an
// eq factor without eq_points); the prover's rule over the proof's table factors and its point (table_rule: n = 1 is
// ZIGZ_ERR_NO_VARIABLES); then the words of the proof and of its taus (ZIGZ_ERR_NOT_CANONICAL).  What a proof holds never makes
// an error, only a word >= p does.  dev, values: as table_rule's.  k == 0 is ZIGZ_OK.
inline zigz_status check_verify_product_batch(const VerifyArgs &a, bool dev, bool values, size_t *bad_index) {
    if (!a.n_rejected || (a.flags & ~(uint32_t)ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED)) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (a.k == 0) return ZIGZ_OK;
    if (a.k > ZIGZ_BATCH_MAX || !a.degrees || !a.factors || !a.ns || !a.claimed_sums || !a.rounds || !a.points || !a.final_evals)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, values, true, true, sv::SV_MAX_LOG2_N};
    size_t foff = 0, voff = 0, roff = 0, eoff = 0;
    for (size_t i = 0; i < a.k; i++) {
        const unsigned d = a.degrees[i];
        if (d < 1 || d > MAX_DEGREE) return fail_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const void *tables[MAX_DEGREE];
        unsigned nt = 0, neq = 0;
        for (unsigned j = 0; j < d; j++) {
            const uint8_t kind = kind_of(a, foff + j);
            if (kind == KIND_TABLE) {
                tables[nt++] = a.factors[foff + j];
            } else if (kind != KIND_EQ || a.factors[foff + j] || !a.eq_points) {
                return fail_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
            } else {
                neq++;
            }
        }
        const zigz_status st = table_rule(rule, tables, nt, a.ns[i], a.points + voff);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        const size_t v = log2_floor(a.ns[i]);
        if (!canonical(a.rounds + roff, (d + 1) * v) || a.claimed_sums[i] >= ZIGZ_BABYBEAR_P || a.final_evals[i] >= ZIGZ_BABYBEAR_P ||
            (a.factor_evals && !canonical(a.factor_evals + foff, d)) || (neq && !canonical(a.eq_points + eoff, neq * v)))
            return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        foff += d;
        voff += v;
        roff += (d + 1) * v;
        eoff += neq * v;
    }
    return ZIGZ_OK;
}

// The host form's checks in the family's order (batch_host.hpp: checks_in_call_order): a TABLE factor that holds a value >= p in
// a proof BEFORE the first one that fails another check is reported instead, with its proof.  When every proof passes, the
// caller checks the values while it narrows them.
inline zigz_status check_verify_product_batch_host(const VerifyArgs &a, size_t *bad_index, bool *value_found = nullptr) {
    size_t bad = a.k;
    const zigz_status st = check_verify_product_batch(a, false, false, &bad);
    if (value_found) *value_found = false;
    if (st == ZIGZ_OK || bad >= a.k) return st;
    size_t foff = 0;
    for (size_t i = 0; i < bad; i++)  // (their degrees, kinds and pointers have passed)
        for (unsigned j = 0; j < a.degrees[i]; j++, foff++)
            if (kind_of(a, foff) == KIND_TABLE && !canonical((const uint64_t *)a.factors[foff], a.ns[i])) {
                if (value_found) *value_found = true;
                return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
            }
    return fail_at(bad_index, bad, st);
}

// sv::replay_rounds with d + 1 coefficients c_0..c_d per round (verifyRounds, sumcheck_verifier.zig:172-205): g(0) + g(1) =
// 2 c_0 + c_1 + .. + c_d must equal the claim, the coefficients are absorbed in order, the challenge is drawn and the claim
// becomes g(challenge) by Horner.  d = 1 gives sv::replay_rounds' Replay word for word.
inline sv::Replay replay_rounds(uint64_t claimed_sum, const uint64_t *rounds, size_t v, unsigned d) {
    Transcript tr;
    uint64_t claim = claimed_sum;
    for (size_t r = 0; r < v; r++) {
        const uint64_t *c = rounds + (size_t)(d + 1) * r;
        uint64_t s = c[0];
        for (unsigned j = 0; j <= d; j++) s = f_add(s, c[j]);
        if (s != claim) return sv::Replay{false, claim};
        const uint64_t ch = absorb_and_draw(tr, c, d + 1);
        claim = c[d];
        for (unsigned j = d; j > 0; j--) claim = f_add(f_mul(claim, ch), c[j - 1]);
    }
    return sv::Replay{true, claim};
}

// the multilinear extension of eq(tau, .) at q, prod_j (tau_j q_j + (1 - tau_j)(1 - q_j)): v field elements in, no table.
// reversed: q_j is q[v - 1 - j] (the point of a proof read back to front, where the prover's evaluations live)
inline uint64_t eq_at(const uint64_t *tau, const uint64_t *q, size_t v, bool reversed = false) {
    uint64_t w = 1;
    for (size_t j = 0; j < v; j++) {
        const uint64_t t = tau[j], x = q[reversed ? v - 1 - j : j];
        w = f_mul(w, f_add(f_mul(t, x), f_mul(f_sub(1, t), f_sub(1, x))));
    }
    return w;
}

// the final check once the d oracles' evaluations are known: their product equals the last claim and final_eval, and (when the
// proof's factor evals are checked) every oracle its factor eval
inline uint8_t verdict(const sv::Replay &r, const uint64_t *oracle_evals, unsigned d, uint64_t final_eval, const uint64_t *factor_evals) {
    uint64_t prod = oracle_evals[0];
    for (unsigned j = 1; j < d; j++) prod = f_mul(prod, oracle_evals[j]);
    bool ok = r.rounds_ok && prod == r.expected && prod == final_eval;
    if (factor_evals)
        for (unsigned j = 0; j < d; j++) ok = ok && oracle_evals[j] == factor_evals[j];
    return ok ? 1 : 0;
}

}  // namespace pv
}  // namespace zk
