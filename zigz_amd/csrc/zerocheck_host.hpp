#pragma once
// The host side of the zero-check sumcheck with the eq factor in closed form (api_zerocheck.cpp, sumcheck_zerocheck.hip; DESIGN.md
// s7j): instance i proves
//   S_i = sum_x eq(tau_i, x) C_i(x),   C_i(x) = sum_{t < T_i} alpha_t prod_{j < d_t} pool[idx(t, j)](x),
// over a pool of M_i tables none of which is eq.  The bind is MSB-first, so round r binds index bit v - 1 - r, which is tau_{v-1-r}'s
// (tau[0] goes with the LSB, as in zigz_dev_eq_table_batch), and the weight factors without a division:
//   s_r(X) = P_r ((1 - tau_j) + (2 tau_j - 1) X) t_r(X),   j = v - 1 - r,   P_r = prod_{r' < r} eq(tau_{v-1-r'}, c_r'),
//   t_r(X) = sum_{x < m/2} W_r[x] sum_t alpha_t prod_j (a_j[x] + X (b_j[x] - a_j[x])),   W_r = eq(tau_0 .. tau_{v-r-2}, .).
// t_r has the degree D of C; s_r has D + 2 coefficients.  Here: the argument rules of the four entries, the prefix scalar P_r, the
// multiplication by the linear factor, the weights the kernels read -- W_r[x] = lo[x & (2^L - 1)] hi_r[x >> L], lo the eq table of
// tau_0..tau_{L-1} and hi_r the stages of eq(tau_L.., .) built by doubling, their room per instance and the stage a pass reads
// (weight_words, stage) --, the rounds of an instance that has become small
// enough for the host, and the verifier's verdict.  On top of sop_host.hpp (layout, terms, class sums -> coefficients).  Plain
// C++, no HIP: testable without a GPU (tests/c_driver/zerocheck_host.cpp).
#include "sop_host.hpp"

namespace zk {
namespace zc {

constexpr unsigned MAX_DEGREE = ZIGZ_ZEROCHECK_MAX_DEGREE;  // of a round polynomial: deg C + 1
static_assert(MAX_DEGREE == sop::MAX_DEGREE + 1, "the eq factor adds one to the degree of C");
// The kernels' split of a pair index: the low LOG2_LO bits choose the word of `lo`, the rest the word of the round's `hi` stage.
// A live round has at least 1024 pairs (m >= 2048), so with 2^LOG2_LO == 1024 the split holds at every live length.
constexpr unsigned LOG2_LO = 10;
static_assert(((size_t)1 << LOG2_LO) == HOST_TAIL_MAX, "the smallest live round has exactly 2^LOG2_LO pairs");

// eq(t, c) = t c + (1 - t)(1 - c)
inline uint64_t eq1(uint64_t t, uint64_t c) { return f_add(f_mul(t, c), f_mul(f_sub(1, t), f_sub(1, c))); }

// eq(tau_0 .. tau_{s-1}, .): 2^s canonical words, tau[0] with the LSB of the index (zerocheck tables are built the same way)
inline std::vector<uint64_t> eq_prefix(const uint64_t *tau, unsigned s) {
    std::vector<uint64_t> e((size_t)1 << s);
    e[0] = 1;
    for (unsigned j = 0; j < s; j++) {
        const size_t h = (size_t)1 << j;
        const uint64_t t = tau[j], nt = f_sub(1, tau[j]);
        for (size_t x = 0; x < h; x++) {
            e[x + h] = f_mul(e[x], t);
            e[x] = f_mul(e[x], nt);
        }
    }
    return e;
}

// a canonical word in Montgomery form (x R mod p), as the kernels multiply it in
inline uint32_t mont(uint64_t x) { return (uint32_t)f_mul(x, pd::R1); }

// The weights of an instance of v > L variables as the passes read them, in Montgomery form: lo (2^L words) and the stages of hi
// one behind the other -- stage s = eq(tau_L .. tau_{L+s-1}, .), 2^s words, starts at word stage_at(s); stages 0 .. v - L - 1.
// The round with 2^(L + s) pairs reads stage s.  words(v, L) words in all, fewer than 2^L + 2^(v - L).
inline size_t stage_at(unsigned s) { return ((size_t)1 << s) - 1; }
inline size_t hi_words(unsigned v, unsigned L) { return ((size_t)1 << (v - L)) - 1; }
// A live instance's words in a call's weights region: lo and the stages of hi, rounded up so that the next instance's lo is
// 16-byte aligned
inline size_t weight_words(size_t n) { return ((size_t)1 << LOG2_LO) + (((size_t)1 << (log2_floor(n) - LOG2_LO)) + 3) / 4 * 4; }
// A pass over tables of m values sums for the round with pairs(m, bind) index pairs -- m / 2 in round 0, m / 4 behind a bind -- and
// reads stage log2(pairs) - LOG2_LO of hi (a bind at m == 2048 sums for nobody: stage 0, one valid word)
inline size_t pairs(size_t m, bool bind) { return bind ? m / 4 : m / 2; }
inline unsigned stage(size_t m, bool bind) {
    const size_t p = pairs(m, bind);
    return p >= ((size_t)1 << LOG2_LO) ? log2_floor(p) - LOG2_LO : 0;
}
inline void build_weights(const uint64_t *tau, unsigned v, unsigned L, uint32_t *lo, uint32_t *hi) {
    const std::vector<uint64_t> e = eq_prefix(tau, L);
    for (size_t x = 0; x < e.size(); x++) lo[x] = mont(e[x]);
    std::vector<uint64_t> st(1, 1);
    for (unsigned s = 0;; s++) {  // (each stage is the one before it doubled by the next tau)
        for (size_t x = 0; x < st.size(); x++) hi[stage_at(s) + x] = mont(st[x]);
        if (s + 1 >= v - L) break;
        const uint64_t t = tau[L + s], nt = f_sub(1, tau[L + s]);
        st.resize(st.size() * 2);
        for (size_t x = 0; x < st.size() / 2; x++) {
            st[x + st.size() / 2] = f_mul(st[x], t);
            st[x] = f_mul(st[x], nt);
        }
    }
}

// The scalar side of one instance's weight: P_r and the linear factor of the round
struct Weight {
    const uint64_t *tau = nullptr;
    size_t v = 0;
    uint64_t P = 1;  // prod over the rounds so far of eq(tau_{v-1-r'}, c_r')

    // round r: the D + 1 coefficients of t_r -> the D + 2 coefficients of s_r = P_r ((1 - tau_j) + (2 tau_j - 1) X) t_r
    void round_poly(size_t r, unsigned D, const uint64_t *t, uint64_t *s) const {
        const uint64_t tj = tau[v - 1 - r];
        const uint64_t l0 = f_mul(P, f_sub(1, tj)), l1 = f_mul(P, f_sub(f_add(tj, tj), 1));
        s[0] = f_mul(l0, t[0]);
        for (unsigned j = 1; j <= D; j++) s[j] = f_add(f_mul(l0, t[j]), f_mul(l1, t[j - 1]));
        s[D + 1] = f_mul(l1, t[D]);
    }
    void bound(size_t r, uint64_t ch) { P = f_mul(P, eq1(tau[v - 1 - r], ch)); }
    // one round from t_r: records s_r, draws (or takes) the challenge, moves P on
    uint64_t step(SumcheckRounds &pr, unsigned D, const uint64_t *t) {
        uint64_t s[MAX_DEGREE + 1];
        const size_t r = pr.round;
        round_poly(r, D, t, s);
        const uint64_t ch = pr.step(s);
        if (pr.st == ZIGZ_OK) bound(r, ch);
        return ch;
    }
};

// sop::tail_rounds under the weight: t_r from W_r built afresh for every round (m / 2 words); pr.ncoef is D + 2 and pr.round the
// rounds already run.  Returns sop::combine() of the fully bound tables -- C at the point, WITHOUT the eq factor.
struct Weighted {
    static constexpr bool WEIGHTED = true;
    Weight &w;
    unsigned D;
    std::vector<uint64_t> begin_round(size_t half) { return eq_prefix(w.tau, log2_floor(half)); }
    uint64_t step(SumcheckRounds &pr, const uint64_t *c) { return w.step(pr, D, c); }
};
inline uint64_t tail_rounds(SumcheckRounds &pr, Weight &w, std::vector<uint64_t> *pool, unsigned M, const sop::Term *terms, unsigned T,
                            unsigned D, uint64_t *table_evals = nullptr) {
    Weighted wt{w, D};
    return sop::tail_rounds_of(pr, wt, pool, M, terms, T, table_evals);
}

// ------------------------------------------------------------------ the prover's arguments
// zigz_[dev_]sumcheck_prove_zerocheck_batch: the sop entry's arguments, eq_points (sum v_i words) and eq_evals[k]
struct Args {
    sop::Args s;
    const uint64_t *eq_points;
    const void *eq_evals;
};

// instance i's first round word: D_i + 2 coefficients per round
inline std::vector<size_t> round_offsets(const std::vector<sop::Shape> &sh) {
    std::vector<size_t> roff(sh.size() + 1, 0);
    for (size_t i = 0; i < sh.size(); i++) roff[i + 1] = roff[i] + (size_t)(sh[i].D + 2) * sh[i].nv;
    return roff;
}

// the first instance in front of `limit` whose tau holds a word >= p, or `limit` (the instances in front of `limit` have
// passed the sop rule: their lengths are powers of two)
inline size_t first_bad_tau(const Args &a, size_t limit) {
    size_t voff = 0;
    for (size_t i = 0; i < limit; i++) {
        const size_t v = log2_floor(a.s.ns[i]);
        if (!canonical(a.eq_points + voff, v)) return i;
        voff += v;
    }
    return limit;
}

// What the entries say about their arguments before anything runs: sop::check_sop_batch's statuses in its order, and per
// instance, after its coefficients, ZIGZ_ERR_NOT_CANONICAL for a tau word >= p; eq_points or eq_evals NULL is
// ZIGZ_ERR_INVALID_ARGUMENT.  The first failing instance's index goes to *bad_index.  k == 0 is ZIGZ_OK.
inline zigz_status check_zerocheck_batch(const Args &a, bool dev, bool values, size_t *bad_index, size_t *first_table = nullptr) {
    if (a.s.k == 0) return ZIGZ_OK;
    if (!a.eq_points || !a.eq_evals) return ZIGZ_ERR_INVALID_ARGUMENT;
    size_t bad = a.s.k;
    const zigz_status st = sop::check_sop_batch(a.s, dev, values, &bad, first_table);
    if (st != ZIGZ_OK && bad >= a.s.k) return st;  // not an instance's failure
    const size_t t = first_bad_tau(a, bad);
    if (t < bad) {
        if (first_table) {
            *first_table = 0;
            for (size_t i = 0; i < t; i++) *first_table += a.s.n_tables[i];
        }
        return fail_at(bad_index, t, ZIGZ_ERR_NOT_CANONICAL);
    }
    return st == ZIGZ_OK ? st : fail_at(bad_index, bad, st);
}

// The host form's checks in the family's order: a table holding a value >= p in an instance BEFORE the first one that fails
// another check is reported instead, with its instance.
inline zigz_status check_zerocheck_batch_host(const Args &a, size_t *bad_index, bool *value_found = nullptr) {
    if (value_found) *value_found = false;
    if (a.s.k == 0) return ZIGZ_OK;
    if (!a.eq_points || !a.eq_evals) return ZIGZ_ERR_INVALID_ARGUMENT;
    size_t bad = a.s.k;
    const zigz_status st = sop::check_sop_batch_host(a.s, &bad, value_found);
    if (st != ZIGZ_OK && bad >= a.s.k) return st;
    const size_t t = first_bad_tau(a, bad);
    if (t >= bad) return st == ZIGZ_OK ? st : fail_at(bad_index, bad, st);
    size_t moff = 0;
    for (size_t i = 0; i < t; i++)
        for (unsigned j = 0; j < a.s.n_tables[i]; j++, moff++)
            if (!canonical((const uint64_t *)a.s.tables[moff], a.s.ns[i])) {
                if (value_found) *value_found = true;
                return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
            }
    if (value_found) *value_found = false;
    return fail_at(bad_index, t, ZIGZ_ERR_NOT_CANONICAL);
}

// ------------------------------------------------------------------ verification
// The arguments of zigz_[dev_]sumcheck_verify_zerocheck_batch: the prover's layout; table_evals and eq_evals may be NULL
struct VerifyArgs {
    size_t k;
    const unsigned *n_tables;
    const void *const *tables;
    const uint64_t *eq_points;
    const size_t *ns;
    const unsigned *n_terms, *term_degrees;
    const uint8_t *term_tables;
    const uint64_t *term_coeffs;
    const uint64_t *claimed_sums, *rounds, *points, *table_evals, *eq_evals, *final_evals;
    uint32_t flags;
    const size_t *n_rejected;
};

// What the entries say about their arguments before anything runs: sop::verify_walk with D_i + 2 words per round, every pool
// entry a table, eq_points required, and a proof's tau (its v words of eq_points) and eq_eval canonical.
inline zigz_status check_verify_zerocheck_batch(const VerifyArgs &a, bool dev, bool values, size_t *bad_index) {
    if (a.k && !a.eq_points) return ZIGZ_ERR_INVALID_ARGUMENT;  // (as every other failure in front of the proofs)
    size_t voff = 0;
    return sop::verify_walk(
        a, dev, values, 2, bad_index, [](size_t) { return 1; },
        [&](size_t i, size_t v, unsigned) {
            if ((a.eq_evals && a.eq_evals[i] >= ZIGZ_BABYBEAR_P) || !canonical(a.eq_points + voff, v)) return false;
            voff += v;
            return true;
        });
}
inline zigz_status check_verify_zerocheck_batch_host(const VerifyArgs &a, size_t *bad_index, bool *value_found = nullptr) {
    size_t bad = a.k;
    const zigz_status st = check_verify_zerocheck_batch(a, false, false, &bad);
    return sop::verify_walk_host(a, st, bad, bad_index, value_found, [](size_t) { return true; });
}

// the final check once the M tables' evaluations and eq's are known: eq * C(oracles) equals the last claim and final_eval, and
// every given eval its oracle
inline uint8_t verdict(const sv::Replay &r, const sop::Term *terms, unsigned T, const uint64_t *oracle_evals, unsigned M, uint64_t eq_oracle,
                       uint64_t final_eval, const uint64_t *table_evals, const uint64_t *eq_eval) {
    const uint64_t o = f_mul(eq_oracle, sop::combine(terms, T, oracle_evals));
    bool ok = r.rounds_ok && o == r.expected && o == final_eval;
    if (table_evals)
        for (unsigned j = 0; j < M; j++) ok = ok && oracle_evals[j] == table_evals[j];
    if (eq_eval) ok = ok && eq_oracle == *eq_eval;
    return ok ? 1 : 0;
}

}  // namespace zc
}  // namespace zk
