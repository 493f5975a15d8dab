#pragma once
// The host side of the batched MLE evaluation and the batched sumcheck verification (api_mle_batch.cpp): the
// argument checks of the four entries and the replay of a proof's rounds (SumcheckVerifier.verify / verifyRounds,
// src/proofs/sumcheck_verifier.zig:48-108,172-205) with the library's own transcript.  Plain C++, no HIP: the header is
// testable without a GPU (tests/c_driver/sumcheck_verify_host.cpp), like open_plan.hpp and verify_plan.hpp.
#include <stddef.h>
#include <stdint.h>

#include "batch_host.hpp"  // canonical()
#include "host_hash.hpp"
#include "zigz_hip.h"

namespace zk {
namespace sv {

constexpr uint64_t SV_P = ZIGZ_BABYBEAR_P;
constexpr unsigned SV_MAX_LOG2_N = 32;  // the batched eval's exact u64 sum: 2^31 * n < 2^64 (mle_batch.hip)

inline uint64_t f_add(uint64_t a, uint64_t b) { const uint64_t s = a + b; return s >= SV_P ? s - SV_P : s; }
inline uint64_t f_mul(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) % SV_P); }
inline unsigned log2_of(size_t n) { unsigned l = 0; while (n > 1) { n >>= 1; l++; } return l; }
inline zigz_status bad_at(size_t *bad_index, size_t i, zigz_status st) {
    if (bad_index) *bad_index = i;
    return st;
}
// Multilinear.init (multilinear.zig:36-44), and the largest table the batched eval sums exactly
inline zigz_status shape(size_t n) {
    if (n == 0) return ZIGZ_ERR_EMPTY_EVALUATIONS;
    if (n & (n - 1)) return ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO;
    if (log2_of(n) > SV_MAX_LOG2_N) return ZIGZ_ERR_INVALID_ARGUMENT;
    return ZIGZ_OK;
}

// What zigz_[dev_]mle_eval_batch says about its arguments before anything runs: ZIGZ_OK, or the status the single entry
// (zigz_dev_mle_eval / zigz_mle_eval with point_len = log2 n) would return for the first pair it rejects, whose index goes to
// *bad_index.  dev: the tables are device pointers (16-byte aligned, never read here); otherwise host tables, whose values are
// checked when `values` is set (the library checks them while it narrows them instead).  k == 0 is ZIGZ_OK.
inline zigz_status check_eval_batch(const void *const *tables, const size_t *ns, size_t k, const uint64_t *points, const void *out,
                                    bool dev, bool values, size_t *bad_index) {
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !tables || !ns || !out) return ZIGZ_ERR_INVALID_ARGUMENT;
    size_t off = 0;
    for (size_t i = 0; i < k; i++) {
        if (dev && !tables[i]) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const zigz_status st = shape(ns[i]);
        if (st != ZIGZ_OK) return bad_at(bad_index, i, st);
        const size_t v = log2_of(ns[i]);
        if (!tables[i] || (v && !points)) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        if (dev && ((uintptr_t)tables[i] & 15)) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        if (!dev && values && !canonical((const uint64_t *)tables[i], ns[i])) return bad_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        if (v && !canonical(points + off, v)) return bad_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        off += v;
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
    size_t off = 0;
    for (size_t i = 0; i < k; i++) {
        if (dev && !tables[i]) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const zigz_status st = shape(ns[i]);
        if (st != ZIGZ_OK) return bad_at(bad_index, i, st);
        if (ns[i] == 1) return bad_at(bad_index, i, ZIGZ_ERR_NO_VARIABLES);
        if (!tables[i]) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        if (dev && ((uintptr_t)tables[i] & 15)) return bad_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
        const size_t v = log2_of(ns[i]);
        if ((!dev && values && !canonical((const uint64_t *)tables[i], ns[i])) || !canonical(points + off, v) ||
            !canonical(rounds + 2 * off, 2 * v) || claimed_sums[i] >= SV_P || final_evals[i] >= SV_P)
            return bad_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        off += v;
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
        tr.append_field(c0);
        tr.append_field(c1);
        claim = f_add(f_mul(c1, tr.challenge()), c0);
    }
    return Replay{true, claim};
}
// the final check (:96-100) once the oracle's evaluation is known
inline uint8_t verdict(const Replay &r, uint64_t oracle_eval, uint64_t final_eval) {
    return r.rounds_ok && oracle_eval == r.expected && oracle_eval == final_eval ? 1 : 0;
}

}  // namespace sv
}  // namespace zk
