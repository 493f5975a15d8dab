#pragma once
// The host side of the radix sumcheck (DESIGN.md "the radix sumcheck", s7b), shared by the single-table prover (radix_run,
// api_mle.cpp, also sharded by rows) and the batched one (radix_run_batch, api_batch.cpp): the stage rule, the host field
// arithmetic and one table's rounds with its own transcript.  Both provers run every table through this code, so a table's
// rounds, point and final_eval are the same whichever of them proves it.
#include "api_internal.hpp"

// k of the next stage of a table of len entries (the block sums of 2^k blocks): min(log2 len - 8, RADIX_MAX_K) while
// len > HOST_TAIL_MAX; 0 once the table is small enough for the host tail
inline unsigned radix_stage_k(size_t len) {
    if (len <= HOST_TAIL_MAX) return 0;
    const unsigned l = log2_floor(len);
    return l - 8 < RADIX_MAX_K ? l - 8 : RADIX_MAX_K;
}

inline uint64_t h_add(uint64_t a, uint64_t b) { uint64_t s = a + b; return s >= P ? s - P : s; }
inline uint64_t h_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + P - b; }
inline uint64_t h_mul(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) % P); }

// One table's prover: its transcript, round counter and outputs.  A step that fails sets st and stops; the caller checks st.
struct RadixProver {
    size_t len = 0;  // current (local) length of the table
    unsigned k = 0;  // the stage being run
    size_t round = 0, nv = 0;
    uint64_t *rounds = nullptr, *point = nullptr;
    const uint64_t *fixed = nullptr;  // caller-fixed challenges, or none: drawn from the transcript
    Transcript tr;                    // fresh per table, sumcheck_protocol.zig:161
    std::vector<uint64_t> B, W;       // the stage's block sums; the eq weights of its challenges
    zigz_status st = ZIGZ_OK;

    // generateChallenge, sumcheck_protocol.zig:176-184: records the round polynomial [c0, c1], then takes the fixed challenge or
    // draws one.  A fixed challenge >= p fails with NOT_CANONICAL before the point is written.
    uint64_t challenge(uint64_t c0, uint64_t c1) {
        rounds[2 * round] = c0;
        rounds[2 * round + 1] = c1;
        uint64_t ch;
        if (fixed) {
            ch = fixed[round];
            if (ch >= P) {
                st = ZIGZ_ERR_NOT_CANONICAL;
                return 0;
            }
        } else {
            tr.append_field(c0);
            tr.append_field(c1);
            ch = tr.challenge();
        }
        point[round++] = ch;
        return ch;
    }
    // k rounds on the block-sums table B (MSB-first, like partialEval); leaves the eq weights of the k challenges in W
    void stage_rounds() {
        for (auto &b : B) b %= P;
        W.assign(1, 1);
        for (unsigned j = 0; j < k; j++) {
            const size_t half = B.size() / 2;
            uint64_t s0 = 0, s1 = 0;
            for (size_t x = 0; x < half; x++) { s0 = h_add(s0, B[x]); s1 = h_add(s1, B[x + half]); }
            const uint64_t ch = challenge(s0, h_sub(s1, s0));
            if (st != ZIGZ_OK) return;
            for (size_t x = 0; x < half; x++) B[x] = h_add(B[x], h_mul(ch, h_sub(B[x + half], B[x])));
            B.resize(half);
            std::vector<uint64_t> W2(W.size() * 2);
            const uint64_t one_minus = h_sub(1, ch);
            for (size_t x = 0; x < W.size(); x++) { W2[2 * x] = h_mul(W[x], one_minus); W2[2 * x + 1] = h_mul(W[x], ch); }
            W.swap(W2);
        }
    }
    // the last rounds on the remaining (<= 1024 entries per rank) table; returns final_eval
    uint64_t tail_rounds(std::vector<uint64_t> &tail) {
        while (tail.size() > 1) {
            const size_t half = tail.size() / 2;
            uint64_t s0 = 0, s1 = 0;
            for (size_t x = 0; x < half; x++) { s0 = h_add(s0, tail[x]); s1 = h_add(s1, tail[x + half]); }
            const uint64_t ch = challenge(s0, h_sub(s1, s0));
            if (st != ZIGZ_OK) return 0;
            for (size_t x = 0; x < half; x++) tail[x] = h_add(tail[x], h_mul(ch, h_sub(tail[x + half], tail[x])));
            tail.resize(half);
        }
        if (round != nv) st = ZIGZ_ERR_PROTOCOL_ERROR;  // sumcheck_prover.zig:80-82
        return tail.empty() ? 0 : tail[0];
    }
};
