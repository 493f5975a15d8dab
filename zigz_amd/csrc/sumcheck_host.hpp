#pragma once
// The host side of every sumcheck entry: the BabyBear field helpers, Multilinear.init's shape rule, the
// per-table argument rule of the batched entries, the Fiat-Shamir round step, the rounds of a table that has become small enough
// for the host, and the radix schedules -- one table (radix_run, also sharded by rows) and many (radix_run_batch) -- as
// orchestration over caller-supplied data passes.  The linear provers (api_mle.cpp, api_batch.cpp), the product prover
// (api_product.cpp, product_host.hpp) and the verifier's replay (sumcheck_verify_host.hpp) all run this code, so a table's rounds,
// point and final_eval are the same whichever of them handles it.  Plain C++, no HIP: testable without a GPU
// (tests/c_driver/radix_host.cpp, product_host.cpp, sumcheck_verify_host.cpp).
#include <stdint.h>

#include <vector>

#include "batch_host.hpp"  // canonical()
#include "host_hash.hpp"
#include "host_parallel.hpp"
#include "zigz_hip.h"

namespace zk {

constexpr unsigned SUMCHECK_MAX_DEGREE = ZIGZ_PRODUCT_MAX_DEGREE;
constexpr unsigned RADIX_MAX_K = 10;    // 1024 block sums per radix sumcheck stage
constexpr size_t HOST_TAIL_MAX = 1024;  // a table this long or shorter finishes its rounds on the host (every prover's hand-over)

inline uint64_t f_add(uint64_t a, uint64_t b) { const uint64_t s = a + b; return s >= ZIGZ_BABYBEAR_P ? s - ZIGZ_BABYBEAR_P : s; }
inline uint64_t f_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + ZIGZ_BABYBEAR_P - b; }
inline uint64_t f_mul(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) % ZIGZ_BABYBEAR_P); }
inline unsigned log2_floor(size_t n) { unsigned l = 0; while (n > 1) { n >>= 1; l++; } return l; }

// a batched entry's failure at entry i: i into *bad_index (when asked for), the status returned
inline zigz_status fail_at(size_t *bad_index, size_t i, zigz_status st) {
    if (bad_index) *bad_index = i;
    return st;
}
// Multilinear.init, multilinear.zig:36-44
inline zigz_status mle_check(size_t n) {
    if (n == 0) return ZIGZ_ERR_EMPTY_EVALUATIONS;
    if (n & (n - 1)) return ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO;
    return ZIGZ_OK;
}

// What a batched entry says about ONE of its instances -- d tables of n values and the log2 n words that go with them (fixed
// challenges, or the coordinates of a point) -- in the order the single entries answer: a null device pointer, the shape, n = 1,
// a null pointer, the alignment, the values, the words.  dev: device pointers (16-byte aligned, never read here); otherwise host
// tables, whose values are checked when `values` is set (the library checks them while it narrows them instead).
struct TableRule {
    bool dev, values;
    bool no_variables;    // n = 1 is ZIGZ_ERR_NO_VARIABLES (the provers and the verifier; an evaluation has a value)
    bool words_required;  // words == nullptr is an error where there are variables (otherwise: no words given)
    unsigned max_log2_n;  // the family's largest table (its exact u64 sums)
};
inline zigz_status table_rule(const TableRule &r, const void *const *tables, unsigned d, size_t n, const uint64_t *words) {
    if (r.dev)
        for (unsigned j = 0; j < d; j++)
            if (!tables[j]) return ZIGZ_ERR_INVALID_ARGUMENT;
    const zigz_status st = mle_check(n);
    if (st != ZIGZ_OK) return st;
    const size_t v = log2_floor(n);
    if (v > r.max_log2_n) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (r.no_variables && n == 1) return ZIGZ_ERR_NO_VARIABLES;
    if (r.words_required && v && !words) return ZIGZ_ERR_INVALID_ARGUMENT;
    for (unsigned j = 0; j < d; j++)
        if (!tables[j] || (r.dev && ((uintptr_t)tables[j] & 15))) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (!r.dev && r.values)
        for (unsigned j = 0; j < d; j++)
            if (!canonical((const uint64_t *)tables[j], n)) return ZIGZ_ERR_NOT_CANONICAL;
    if (words && !canonical(words, v)) return ZIGZ_ERR_NOT_CANONICAL;
    return ZIGZ_OK;
}

// generateChallenge's transcript half (sumcheck_protocol.zig:176-184): absorbs a round's coefficients in order and draws
inline uint64_t absorb_and_draw(Transcript &tr, const uint64_t *c, unsigned ncoef) {
    for (unsigned j = 0; j < ncoef; j++) tr.append_field(c[j]);
    return tr.challenge();
}

// One instance's prover: its transcript, round counter and outputs.  A step that fails sets st and stops; the caller checks st.
struct SumcheckRounds {
    unsigned ncoef = 2;  // coefficients per round: the degree of the round polynomial + 1
    size_t round = 0, nv = 0;
    uint64_t *rounds = nullptr, *point = nullptr;
    uint64_t *claimed_sum = nullptr;  // when set: receives the first round's g(0) + g(1)
    const uint64_t *fixed = nullptr;  // caller-fixed challenges, or none: drawn from the transcript
    Transcript tr;                    // fresh per instance, sumcheck_protocol.zig:161
    zigz_status st = ZIGZ_OK;

    // generateChallenge: records the round polynomial c_0 .. c_{ncoef - 1}, then takes the fixed challenge or draws one.  A fixed
    // challenge >= p fails with NOT_CANONICAL after the coefficients are recorded and before the point is written.
    uint64_t step(const uint64_t *c) {
        if (claimed_sum && round == 0) {
            uint64_t s = c[0];
            for (unsigned j = 0; j < ncoef; j++) s = f_add(s, c[j]);
            *claimed_sum = s;
        }
        for (unsigned j = 0; j < ncoef; j++) rounds[ncoef * round + j] = c[j];
        uint64_t ch;
        if (fixed) {
            ch = fixed[round];
            if (ch >= ZIGZ_BABYBEAR_P) {
                st = ZIGZ_ERR_NOT_CANONICAL;
                return 0;
            }
        } else {
            ch = absorb_and_draw(tr, c, ncoef);
        }
        point[round++] = ch;
        return ch;
    }
    // one MSB-first bind (partialEval, multilinear.zig:166-173) of a table of canonical values, in place
    static void bind(std::vector<uint64_t> &t, uint64_t ch) {
        const size_t half = t.size() / 2;
        for (size_t x = 0; x < half; x++) t[x] = f_add(t[x], f_mul(ch, f_sub(t[x + half], t[x])));
        t.resize(half);
    }
    // The last rounds on the remaining tables of d = ncoef - 1 factors (f[j]: m canonical values each, bound in place): g(t) =
    // sum_{i < m/2} prod_j (a_j + t (b_j - a_j)) with a_j = f_j[i], b_j = f_j[i + m/2], the product started from the first factor.
    // One factor: the two half sums and ONE subtraction per round, as roundPolynomial has it (multilinear.zig:228-229).  Writes
    // every factor fully bound (factor_evals, when asked for) and returns their product.
    uint64_t tail_rounds(std::vector<uint64_t> *f, uint64_t *factor_evals = nullptr) {
        return ncoef == 2 ? tail_rounds_of<1>(f, factor_evals) : ncoef == 3 ? tail_rounds_of<2>(f, factor_evals) : tail_rounds_of<3>(f, factor_evals);
    }
    // (the degree is a template argument so that the per-element loops unroll and a round's coefficients stay in registers)
    template <unsigned D>
    uint64_t tail_rounds_of(std::vector<uint64_t> *f, uint64_t *factor_evals) {
        static_assert(D >= 1 && D <= SUMCHECK_MAX_DEGREE, "one to three factors");
        for (size_t m = f[0].size(); m > 1; m /= 2) {
            const size_t half = m / 2;
            uint64_t c[D + 1] = {};
            for (size_t i = 0; i < half; i++) {
                uint64_t g[D + 1] = {f[0][i], D == 1 ? f[0][i + half] : f_sub(f[0][i + half], f[0][i])};
                for (unsigned j = 1; j < D; j++) {  // g *= a + e t
                    const uint64_t a = f[j][i], e = f_sub(f[j][i + half], a);
                    for (unsigned x = j + 1; x > 0; x--) g[x] = f_add(f_mul(g[x], a), f_mul(g[x - 1], e));
                    g[0] = f_mul(g[0], a);
                }
                for (unsigned j = 0; j <= D; j++) c[j] = f_add(c[j], g[j]);
            }
            if (D == 1) c[1] = f_sub(c[1], c[0]);
            const uint64_t ch = step(c);
            if (st != ZIGZ_OK) return 0;
            for (unsigned j = 0; j < D; j++) bind(f[j], ch);
        }
        if (round != nv) st = ZIGZ_ERR_PROTOCOL_ERROR;  // sumcheck_prover.zig:80-82
        if (f[0].empty()) return 0;
        uint64_t fe = f[0][0];
        for (unsigned j = 1; j < D; j++) fe = f_mul(fe, f[j][0]);
        if (factor_evals)
            for (unsigned j = 0; j < D; j++) factor_evals[j] = f[j][0];
        return fe;
    }
};

// ------------------------------------------------------------------ the radix schedule
// k of the next stage of a table of len entries (the block sums of 2^k blocks): min(log2 len - 8, RADIX_MAX_K) while
// len > HOST_TAIL_MAX; 0 once the table is small enough for the host tail
inline unsigned radix_stage_k(size_t len) {
    if (len <= HOST_TAIL_MAX) return 0;
    const unsigned l = log2_floor(len);
    return l - 8 < RADIX_MAX_K ? l - 8 : RADIX_MAX_K;
}

// One table's linear prover in the radix schedule
struct RadixProver : SumcheckRounds {
    size_t len = 0;              // current (local) length of the table
    unsigned k = 0;              // the stage being run
    std::vector<uint64_t> B, W;  // the stage's block sums; the eq weights of its challenges

    // k rounds on the block-sums table B (MSB-first, like partialEval); leaves the eq weights of the k challenges in W
    void stage_rounds() {
        for (auto &b : B) b %= ZIGZ_BABYBEAR_P;
        W.assign(1, 1);
        for (unsigned j = 0; j < k; j++) {
            const size_t half = B.size() / 2;
            uint64_t s0 = 0, s1 = 0;
            for (size_t x = 0; x < half; x++) { s0 = f_add(s0, B[x]); s1 = f_add(s1, B[x + half]); }
            const uint64_t c[2] = {s0, f_sub(s1, s0)};
            const uint64_t ch = step(c);
            if (st != ZIGZ_OK) return;
            bind(B, ch);
            std::vector<uint64_t> W2(W.size() * 2);
            const uint64_t one_minus = f_sub(1, ch);
            for (size_t x = 0; x < W.size(); x++) { W2[2 * x] = f_mul(W[x], one_minus); W2[2 * x + 1] = f_mul(W[x], ch); }
            W.swap(W2);
        }
    }
};

// The radix sumcheck as orchestration over three data passes (zigz_radix_ops: the exact u64 sums of the 2^k contiguous blocks of
// the current local table; its fold with 2^k canonical weights, with the block sums of the result when k_next != 0; the current
// local table) and, when the table is sharded by rows over several GPUs, one exchange hook.  Row sharding: global
// index i lives on rank i mod G at local index i / G, so the MSB-first bind pairs (i, i + n/2) of the first v - log2 G rounds are
// rank-local, the top k index bits of i are the top k bits of the local index -- a rank's block sums are its share of the
// global block sums -- and the fold T'[i'] = sum_b eq_b T[b*m + i'] is rank-local too.  Per stage of k <= 10 rounds the ranks
// exchange 2^k <= 1024 exact u64 partial sums (ONE all-gather, added locally = an all-reduce), and once the local tables are
// <= 1024 entries one all-gather re-assembles the remaining table (local index j of rank g -> global index j*G + g) that every
// rank finishes identically.  2-3 exchanges per proof instead of one per round; transcripts run in lockstep.
using RadixOps = zigz_radix_ops;
struct ShardComm {
    int rank, world;
    zigz_allgather_fn allgather;
    void *user;
    bool sums_global;  // the data passes already return the sums over ALL ranks (reduced on the device: RCCL all-reduce)
};
// what every sharded entry says about its shard: n_local a table's length; world >= 1 ranks, a power of two, `rank` one of
// them; several ranks need a hook; one value in all has no variables
inline zigz_status shard_check(size_t n_local, int rank, int world, bool have_allgather) {
    const zigz_status st = mle_check(n_local);
    if (st != ZIGZ_OK) return st;
    if (world < 1 || rank < 0 || rank >= world || (world & (world - 1)) || (world > 1 && !have_allgather)) return ZIGZ_ERR_INVALID_ARGUMENT;
    return n_local * (size_t)world == 1 ? ZIGZ_ERR_NO_VARIABLES : ZIGZ_OK;
}

// *err (when the exchange fails): the text for the context's last error.  May throw std::bad_alloc.
inline zigz_status radix_run(const RadixOps &ops, size_t n_local, const ShardComm *comm, const uint64_t *fixed, uint64_t *rounds,
                             uint64_t *point, uint64_t *final_eval, const char **err) {
    const size_t world = comm && comm->world > 1 ? (size_t)comm->world : 1;
    RadixProver s;
    s.len = n_local;
    s.nv = log2_floor(n_local) + log2_floor(world);  // (the rank bits are variables too)
    s.rounds = rounds;
    s.point = point;
    s.fixed = fixed;
    std::vector<uint64_t> gather, wire, all;
    // One exchange: every rank contributes `v` (all ranks the same length) behind ONE status word.  A rank whose local pass
    // failed still takes part -- with its status and a zero payload -- so that all ranks leave the proof at the same
    // exchange: the failing rank with its own error, the others with ZIGZ_ERR_COMM (instead of sitting in the transport's
    // timeout while the failed rank has long returned).
    zigz_status local = ZIGZ_OK;
    auto exchange = [&](const std::vector<uint64_t> &v) -> zigz_status {  // gather := world x v
        const size_t n = v.size();
        wire.assign(n + 1, 0);
        wire[0] = (uint64_t)(uint32_t)local;
        if (local == ZIGZ_OK)
            for (size_t i = 0; i < n; i++) wire[1 + i] = v[i];
        all.assign(world * (n + 1), 0);
        if (!comm->allgather || comm->allgather(comm->user, wire.data(), (n + 1) * 8, all.data()) != 0) {
            *err = "sharded sumcheck: the all-gather hook failed";
            return local != ZIGZ_OK ? local : ZIGZ_ERR_COMM;
        }
        gather.resize(world * n);
        bool peer_failed = false;
        for (size_t r = 0; r < world; r++) {
            if (all[r * (n + 1)] != ZIGZ_OK) peer_failed = true;
            for (size_t i = 0; i < n; i++) gather[r * n + i] = all[r * (n + 1) + 1 + i];
        }
        if (local != ZIGZ_OK) return local;
        if (peer_failed) {
            *err = "sharded sumcheck: another rank reported an error";
            return ZIGZ_ERR_COMM;
        }
        return ZIGZ_OK;
    };
    // a local data pass: alone, its status is returned at once; sharded, it is carried into the next exchange
    auto local_pass = [&](auto &&pass) {
        if (local == ZIGZ_OK) local = pass();
        return local != ZIGZ_OK && world == 1;
    };
    // partial sums of every rank -> totals (exact: < 2^31 * 2^40 per rank, a few ranks)
    auto sum_over_ranks = [&](std::vector<uint64_t> &v) -> zigz_status {
        if (world == 1 || comm->sums_global) return ZIGZ_OK;
        const zigz_status st = exchange(v);
        if (st != ZIGZ_OK) return st;
        for (size_t i = 0; i < v.size(); i++) {
            uint64_t t = 0;
            for (size_t r = 0; r < world; r++) t += gather[r * v.size() + i];
            v[i] = t;
        }
        return ZIGZ_OK;
    };
    zigz_status st;
    if ((s.k = radix_stage_k(s.len))) {
        s.B.assign((size_t)1 << s.k, 0);
        if (local_pass([&] { return ops.block_sums(ops.user, s.k, s.B.data()); })) return local;
        if ((st = sum_over_ranks(s.B)) != ZIGZ_OK) return st;
        for (;;) {
            s.stage_rounds();
            if (s.st != ZIGZ_OK) return s.st;
            const size_t m = s.len >> s.k;
            const unsigned k_next = radix_stage_k(m);
            s.B.assign(k_next ? (size_t)1 << k_next : 0, 0);
            if (local_pass([&] { return ops.fold(ops.user, s.k, s.W.data(), k_next, k_next ? s.B.data() : nullptr); })) return local;
            s.len = m;
            if (!k_next) break;
            if ((st = sum_over_ranks(s.B)) != ZIGZ_OK) return st;
            s.k = k_next;
        }
    }
    // the remaining table: len local entries per rank, global index j*G + g
    const size_t len = s.len;
    std::vector<uint64_t> mine(len), tail;
    if (local_pass([&] { return ops.read_tail(ops.user, len, mine.data()); })) return local;
    if (world == 1) {
        tail.swap(mine);
    } else {
        if ((st = exchange(mine)) != ZIGZ_OK) return st;
        tail.resize(world * len);
        for (size_t r = 0; r < world; r++)
            for (size_t j = 0; j < len; j++) {
                if (gather[r * len + j] >= ZIGZ_BABYBEAR_P) return ZIGZ_ERR_NOT_CANONICAL;  // (the same verdict on every rank)
                tail[j * world + r] = gather[r * len + j];
            }
    }
    const uint64_t fe = s.tail_rounds(&tail);  // the last rounds on the <= 1024 * G entry table, identical on every rank
    if (s.st != ZIGZ_OK) return s.st;
    *final_eval = fe;
    return ZIGZ_OK;
}

// ------------------------------------------------------------------ ... batched
struct BatchOps {  // the three passes of zigz_sumcheck_radix_run_batch
    void *user;
    zigz_radix_batch_sums_fn block_sums;
    zigz_radix_batch_fold_fn fold;
    zigz_radix_batch_tail_fn read_tail;
};

template <class Prover>
zigz_status first_error(const std::vector<Prover> &t) {
    for (const auto &s : t)
        if (s.st != ZIGZ_OK) return s.st;
    return ZIGZ_OK;
}

// The batched orchestration (the batched radix_run): every GPU pass serves every table still in play, between passes each
// table's rounds run on the host's threads with its own transcript.  ns[i] are powers of two >= 2 (checked by the callers).
// May throw std::bad_alloc.
inline zigz_status radix_run_batch(const BatchOps &ops, size_t k, const size_t *ns, const uint64_t *fixed, uint64_t *rounds,
                                   uint64_t *points, uint64_t *final_evals) {
    std::vector<RadixProver> t(k);
    size_t off = 0;
    for (size_t i = 0; i < k; i++) {
        t[i].len = ns[i];
        t[i].nv = log2_floor(ns[i]);
        t[i].rounds = rounds + 2 * off;
        t[i].point = points + off;
        t[i].fixed = fixed ? fixed + off : nullptr;
        off += t[i].nv;
    }
    std::vector<size_t> live, idx2;
    std::vector<unsigned> ks, knext;
    std::vector<uint64_t> sums, weights;
    zigz_status st;
    for (size_t i = 0; i < k; i++)
        if ((t[i].k = radix_stage_k(ns[i]))) {
            live.push_back(i);
            ks.push_back(t[i].k);
        }
    if (!live.empty()) {
        size_t words = 0;
        for (size_t i : live) words += (size_t)1 << t[i].k;
        sums.assign(words, 0);
        if ((st = ops.block_sums(ops.user, live.size(), live.data(), ks.data(), sums.data())) != ZIGZ_OK) return st;
        size_t o = 0;
        for (size_t i : live) {
            t[i].B.assign(sums.begin() + o, sums.begin() + o + ((size_t)1 << t[i].k));
            o += (size_t)1 << t[i].k;
        }
    }
    while (!live.empty()) {
        parallel_for(live.size(), [&](size_t j) { t[live[j]].stage_rounds(); });
        if ((st = first_error(t)) != ZIGZ_OK) return st;
        size_t sn = 0;
        ks.clear();
        knext.clear();
        weights.clear();
        for (size_t i : live) {
            const unsigned kn = radix_stage_k(t[i].len >> t[i].k);
            ks.push_back(t[i].k);
            knext.push_back(kn);
            weights.insert(weights.end(), t[i].W.begin(), t[i].W.end());
            sn += kn ? (size_t)1 << kn : 0;
        }
        sums.assign(sn, 0);
        st = ops.fold(ops.user, live.size(), live.data(), ks.data(), weights.data(), knext.data(), sn ? sums.data() : nullptr);
        if (st != ZIGZ_OK) return st;
        idx2.clear();
        size_t o = 0;
        for (size_t j = 0; j < live.size(); j++) {
            RadixProver &s = t[live[j]];
            s.len >>= s.k;
            if (!knext[j]) continue;
            s.k = knext[j];
            s.B.assign(sums.begin() + o, sums.begin() + o + ((size_t)1 << s.k));
            o += (size_t)1 << s.k;
            idx2.push_back(live[j]);
        }
        live.swap(idx2);
    }
    // every remaining table in one hand-off
    std::vector<size_t> all(k), ms(k), toff(k + 1, 0);
    for (size_t i = 0; i < k; i++) {
        all[i] = i;
        ms[i] = t[i].len;
        toff[i + 1] = toff[i] + ms[i];
    }
    std::vector<uint64_t> tails(toff[k]);
    if ((st = ops.read_tail(ops.user, k, all.data(), ms.data(), tails.data())) != ZIGZ_OK) return st;
    if (!canonical(tails.data(), toff[k])) return ZIGZ_ERR_NOT_CANONICAL;
    parallel_for(k, [&](size_t i) {
        std::vector<uint64_t> tail(tails.begin() + toff[i], tails.begin() + toff[i + 1]);
        final_evals[i] = t[i].tail_rounds(&tail);
    });
    return first_error(t);
}

}  // namespace zk
