#pragma once
// The host side of the batched MLE evaluation and the batched sumcheck verification (api_mle_batch.cpp): the
// argument checks of the four entries and the replay of a proof's rounds (SumcheckVerifier.verify / verifyRounds,
// src/proofs/sumcheck_verifier.zig:48-108,172-205) with the library's own transcript.  Plain C++, no HIP: the header is
// testable without a GPU (tests/c_driver/sumcheck_verify_host.cpp), like open_plan.hpp and verify_plan.hpp.
#include "sumcheck_host.hpp"

namespace zk {
namespace sv {

constexpr unsigned SV_MAX_LOG2_N = 32;  // the batched eval's exact u64 sum: 2^31 * n < 2^64 (mle_batch.hip)

// What zigz_[dev_]mle_eval_batch says about its arguments before anything runs: ZIGZ_OK, or the status the single entry
// (zigz_dev_mle_eval / zigz_mle_eval with point_len = log2 n) would return for the first pair it rejects, whose index goes to
// *bad_index (sumcheck_host.hpp: table_rule; dev, values as there).  k == 0 is ZIGZ_OK.
inline zigz_status check_eval_batch(const void *const *tables, const size_t *ns, size_t k, const uint64_t *points, const void *out,
                                    bool dev, bool values, size_t *bad_index) {
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !tables || !ns || !out) return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, values, false, true, SV_MAX_LOG2_N};
    for (size_t i = 0, off = 0; i < k; off += log2_floor(ns[i++])) {
        const zigz_status st = table_rule(rule, tables + i, 1, ns[i], points ? points + off : nullptr);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
    }
    return ZIGZ_OK;
}

// The same for zigz_[dev_]sumcheck_verify_batch; the single entry is the prover's (zigz_dev_sumcheck_prove /
// zigz_sumcheck_prove): n = 1 is ZIGZ_ERR_NO_VARIABLES.  What a proof holds never makes an error, only a word >= p does.
inline zigz_status check_verify_batch(const void *const *tables, const size_t *ns, size_t k, const uint64_t *claimed_sums,
                                      const uint64_t *rounds, const uint64_t *points, const uint64_t *final_evals, uint32_t flags,
                                      const size_t *n_rejected, bool dev, bool values, size_t *bad_index) {
    if (!n_rejected || (flags & ~(uint32_t)ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED)) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !tables || !ns || !claimed_sums || !rounds || !points || !final_evals) return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, values, true, true, SV_MAX_LOG2_N};
    for (size_t i = 0, off = 0; i < k; off += log2_floor(ns[i++])) {
        const zigz_status st = table_rule(rule, tables + i, 1, ns[i], points + off);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        if (!canonical(rounds + 2 * off, 2 * log2_floor(ns[i])) || claimed_sums[i] >= ZIGZ_BABYBEAR_P || final_evals[i] >= ZIGZ_BABYBEAR_P)
            return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
    }
    return ZIGZ_OK;
}

// The rounds of one proof (sumcheck_verifier.zig:58-93; verifyRounds :172-205): a fresh transcript, claim = claimed_sum; per
// round g(0) + g(1) must equal the claim, then [c0, c1] is absorbed, the challenge drawn (sumcheck_protocol.zig:176-184) and the
// claim becomes g(challenge).  expected: VerificationResult.expected_eval -- the claim at the failing round, or the final one.
struct Replay {
    bool rounds_ok;
    uint64_t expected;
};
inline Replay replay_rounds(uint64_t claimed_sum, const uint64_t *rounds, size_t v) {
    Transcript tr;
    uint64_t claim = claimed_sum;
    for (size_t r = 0; r < v; r++) {
        const uint64_t c0 = rounds[2 * r], c1 = rounds[2 * r + 1];
        if (f_add(c0, f_add(c1, c0)) != claim) return Replay{false, claim};  // g(0) = c0, g(1) = c1 + c0
        claim = f_add(f_mul(c1, absorb_and_draw(tr, rounds + 2 * r, 2)), c0);
    }
    return Replay{true, claim};
}
// the final check (:96-100) once the oracle's evaluation is known
inline uint8_t verdict(const Replay &r, uint64_t oracle_eval, uint64_t final_eval) {
    return r.rounds_ok && oracle_eval == r.expected && oracle_eval == final_eval ? 1 : 0;
}

}  // namespace sv
}  // namespace zk
