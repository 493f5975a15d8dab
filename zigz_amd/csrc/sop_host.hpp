#pragma once
// The host side of the batched sum-of-products sumcheck (api_sop.cpp, sumcheck_sop.hip): instance i proves
//   S_i = sum_x sum_{t < T_i} alpha_t prod_{j < d_t} pool[idx(t, j)](x)
// over a pool of M_i tables.  Here: how the entries' flat arrays are laid out, their argument checks, the round coefficients from
// the per-degree-class sums the kernels publish, the rounds of an instance whose tables have become small enough for the host --
// SumcheckRounds::tail_rounds generalised to a pool with terms, with one body for these rounds and the zero-check's weighted ones
// (tail_rounds_of) --, the verifying entries' argument walk, shared with zerocheck_host.hpp (verify_walk), and the verifier's
// combination.  The prover's schedule and the verifier's run are product_schedule.hpp's.  An instance's transcript and
// round step are sumcheck_host.hpp's, the replay and eq_at product_verify_host.hpp's.  Plain C++, no HIP: testable without a GPU
// (tests/c_driver/sop_host.cpp).
#include "product_host.hpp"
#include "product_verify_host.hpp"

namespace zk {
namespace sop {

constexpr unsigned MAX_TABLES = ZIGZ_SOP_MAX_TABLES, MAX_TERMS = ZIGZ_SOP_MAX_TERMS, MAX_DEGREE = SUMCHECK_MAX_DEGREE;
// the kernels publish, per instance, the coefficient sums of its terms of degree 1 (2 words), 2 (3) and 3 (4), apart
constexpr unsigned SUMS = 2 + 3 + 4;
constexpr unsigned CLASS_AT[MAX_DEGREE] = {0, 2, 5};

// The prover's arguments as the entries take them.  Per instance i: n_tables[i] = M_i pool tables (tables: sum M_i pointers),
// n_terms[i] = T_i terms; per term its degree (term_degrees: sum T_i) and coefficient (term_coeffs: sum T_i); per factor of a
// term its pool index (term_tables: sum of all d_t bytes, term by term).
struct Args {
    size_t k;
    const unsigned *n_tables;
    const void *const *tables;
    const size_t *ns;
    const unsigned *n_terms, *term_degrees;
    const uint8_t *term_tables;
    const uint64_t *term_coeffs;
    const uint64_t *fixed;
    const void *claimed_sums, *rounds, *points, *table_evals, *final_evals;
};

struct Term {
    uint64_t alpha;
    unsigned d;
    uint8_t idx[MAX_DEGREE];
};
// One instance's shape once its arguments have passed: where its words start in every flat array, and its terms
struct Shape {
    size_t moff = 0, toff = 0, voff = 0, roff = 0;  // first pool table, term, variable (point / challenge word), round word
    unsigned M = 0, T = 0, D = 0, nv = 0;           // D: the largest term degree -- D + 1 coefficients per round
    Term terms[MAX_TERMS];
};
// (the arguments have passed check_sop_batch)
inline std::vector<Shape> shapes(size_t k, const unsigned *n_tables, const size_t *ns, const unsigned *n_terms,
                                 const unsigned *term_degrees, const uint8_t *term_tables, const uint64_t *term_coeffs) {
    std::vector<Shape> out(k);
    size_t moff = 0, toff = 0, xoff = 0, voff = 0, roff = 0;
    for (size_t i = 0; i < k; i++) {
        Shape &s = out[i];
        s.moff = moff;
        s.toff = toff;
        s.voff = voff;
        s.roff = roff;
        s.M = n_tables[i];
        s.T = n_terms[i];
        s.nv = log2_floor(ns[i]);
        for (unsigned t = 0; t < s.T; t++) {
            Term &tm = s.terms[t];
            tm.alpha = term_coeffs[toff + t];
            tm.d = term_degrees[toff + t];
            for (unsigned j = 0; j < tm.d; j++) tm.idx[j] = term_tables[xoff + j];
            xoff += tm.d;
            if (tm.d > s.D) s.D = tm.d;
        }
        moff += s.M;
        toff += s.T;
        voff += s.nv;
        roff += (size_t)(s.D + 1) * s.nv;
    }
    return out;
}

// The pool sizes, term counts, degrees and pool indices of instance i (INVALID_ARGUMENT); *n_factors: its term_tables bytes
inline zigz_status check_terms(unsigned M, unsigned T, const unsigned *degrees, const uint8_t *idx, size_t *n_factors) {
    if (M < 1 || M > MAX_TABLES || T < 1 || T > MAX_TERMS) return ZIGZ_ERR_INVALID_ARGUMENT;
    size_t x = 0;
    for (unsigned t = 0; t < T; t++) {
        if (degrees[t] < 1 || degrees[t] > MAX_DEGREE) return ZIGZ_ERR_INVALID_ARGUMENT;
        for (unsigned j = 0; j < degrees[t]; j++)
            if (idx[x + j] >= M) return ZIGZ_ERR_INVALID_ARGUMENT;
        x += degrees[t];
    }
    *n_factors = x;
    return ZIGZ_OK;
}

// What zigz_[dev_]sumcheck_prove_sop_batch says about its arguments before anything runs: ZIGZ_OK, or the status of the first
// instance it rejects, whose index goes to *bad_index.  Per instance, in order: the pool size, the term count, the terms' degrees
// and pool indices; the product prover's rule over the pool and the fixed challenges (sumcheck_host.hpp: table_rule; dev, values
// as there); the coefficients (ZIGZ_ERR_NOT_CANONICAL).  *first_table (may be NULL): the rejected instance's first entry in
// `tables`.  k == 0 is ZIGZ_OK.
inline zigz_status check_sop_batch(const Args &a, bool dev, bool values, size_t *bad_index, size_t *first_table = nullptr) {
    if (a.k == 0) return ZIGZ_OK;
    if (a.k > ZIGZ_BATCH_MAX || !a.n_tables || !a.tables || !a.ns || !a.n_terms || !a.term_degrees || !a.term_tables || !a.term_coeffs ||
        !a.claimed_sums || !a.rounds || !a.points || !a.table_evals || !a.final_evals)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, values, true, false, ZIGZ_PRODUCT_MAX_LOG2_N};
    size_t moff = 0, toff = 0, xoff = 0, voff = 0;
    for (size_t i = 0; i < a.k; i++) {
        if (first_table) *first_table = moff;
        size_t nf = 0;
        zigz_status st = check_terms(a.n_tables[i], a.n_terms[i], a.term_degrees + toff, a.term_tables + xoff, &nf);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        st = table_rule(rule, a.tables + moff, a.n_tables[i], a.ns[i], a.fixed ? a.fixed + voff : nullptr);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        if (!canonical(a.term_coeffs + toff, a.n_terms[i])) return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        moff += a.n_tables[i];
        toff += a.n_terms[i];
        xoff += nf;
        voff += log2_floor(a.ns[i]);
    }
    return ZIGZ_OK;
}

// The host form's checks in the family's order (batch_host.hpp: checks_in_call_order, over the pool tables one behind the other):
// a table holding a value >= p BEFORE the first instance that fails another check is reported instead, with its instance.
inline zigz_status check_sop_batch_host(const Args &a, size_t *bad_index, bool *value_found = nullptr) {
    size_t bad = a.k, ft = 0;
    const zigz_status st = check_sop_batch(a, false, false, &bad, &ft);
    if (value_found) *value_found = false;
    if (st == ZIGZ_OK || bad >= a.k) return st;
    std::vector<size_t> fns, owner;  // the tables in front of the failing instance (their pool sizes and pointers have passed)
    for (size_t i = 0; i < bad; i++)
        for (unsigned j = 0; j < a.n_tables[i]; j++) {
            fns.push_back(a.ns[i]);
            owner.push_back(i);
        }
    size_t fbad = ft;
    const zigz_status st2 = checks_in_call_order((const uint64_t *const *)a.tables, fns.data(), ft + 1, &fbad, [&](size_t *f) {
        *f = ft;
        return st;
    }, value_found);
    if (bad_index) *bad_index = fbad < ft ? owner[fbad] : bad;
    return st2;
}

// the D + 1 canonical coefficients of a round from the SUMS class sums (each below p) the finish launch wrote: class d carries
// R^-d (pd::sum_scale) and contributes to c_0..c_d; a class without terms is all zero
inline void coefficients(unsigned D, const uint64_t *sums, uint64_t *c) {
    for (unsigned j = 0; j <= D; j++) c[j] = 0;
    for (unsigned d = 1; d <= D; d++)
        for (unsigned j = 0; j <= d; j++) c[j] = f_add(c[j], f_mul(sums[CLASS_AT[d - 1] + j], pd::sum_scale(d)));
}

// sum_t alpha_t prod_j evals[idx(t, j)]: final_eval from the tables' evaluations, and the verifier's oracle
inline uint64_t combine(const Term *terms, unsigned T, const uint64_t *evals) {
    uint64_t s = 0;
    for (unsigned t = 0; t < T; t++) {
        uint64_t pr = terms[t].alpha;
        for (unsigned j = 0; j < terms[t].d; j++) pr = f_mul(pr, evals[terms[t].idx[j]]);
        s = f_add(s, pr);
    }
    return s;
}

// a * b mod p for CANONICAL operands: the product is below 2^62, so the reduction is a u64 one (f_mul's 128-bit remainder is
// what the last rounds of a pool of four tables and two terms spent most of their time in)
inline uint64_t mul(uint64_t a, uint64_t b) { return a * b % ZIGZ_BABYBEAR_P; }

// SumcheckRounds::tail_rounds over a pool with terms: the last rounds on the remaining pool tables (pool[j]: m canonical values
// each, bound in place), g(t) = sum_{i < m/2} w_i sum_t alpha_t prod_j (a + t (b - a)) with a = pool[idx][i], b = pool[idx][i + m/2].
// The tables, the coefficients and the challenges are canonical (checked on the way in), so mul() applies.  Writes every pool
// table fully bound (table_evals, when asked for) and returns combine() of them.  `wt` says what a pair weighs and how a round
// steps: Unweighted below (w_i = 1, never multiplied in: the tail is where small instances spend their time), zc::Weighted.
struct Unweighted {
    static constexpr bool WEIGHTED = false;
    std::vector<uint64_t> begin_round(size_t) { return {}; }
    uint64_t step(SumcheckRounds &pr, const uint64_t *c) { return pr.step(c); }
};
template <class Wt>
inline uint64_t tail_rounds_of(SumcheckRounds &pr, Wt &wt, std::vector<uint64_t> *pool, unsigned M, const Term *terms, unsigned T,
                               uint64_t *table_evals) {
    const unsigned D = pr.ncoef - (Wt::WEIGHTED ? 2 : 1);  // (the weighted rounds carry one coefficient more)
    for (size_t m = pool[0].size(); m > 1; m /= 2) {
        const size_t half = m / 2;
        const std::vector<uint64_t> W = wt.begin_round(half);  // the pairs' weights, half of them (none: no weights)
        uint64_t c[MAX_DEGREE + 1] = {};
        for (size_t i = 0; i < half; i++) {
            uint64_t a[MAX_TABLES], e[MAX_TABLES], u[MAX_DEGREE + 1] = {};  // u: the pair's own coefficients, where they are weighed
            for (unsigned j = 0; j < M; j++) {
                a[j] = pool[j][i];
                e[j] = f_sub(pool[j][i + half], a[j]);
            }
            for (unsigned t = 0; t < T; t++) {
                const Term &tm = terms[t];
                uint64_t g[MAX_DEGREE + 1] = {mul(tm.alpha, a[tm.idx[0]]), mul(tm.alpha, e[tm.idx[0]]), 0, 0};
                for (unsigned j = 1; j < tm.d; j++) {  // g *= a + e t
                    const uint64_t aj = a[tm.idx[j]], ej = e[tm.idx[j]];
                    for (unsigned x = j + 1; x > 0; x--) g[x] = f_add(mul(g[x], aj), mul(g[x - 1], ej));
                    g[0] = mul(g[0], aj);
                }
                for (unsigned j = 0; j <= tm.d; j++) {
                    if constexpr (Wt::WEIGHTED)
                        u[j] = f_add(u[j], g[j]);
                    else
                        c[j] = f_add(c[j], g[j]);
                }
            }
            if constexpr (Wt::WEIGHTED)
                for (unsigned j = 0; j <= D; j++) c[j] = f_add(c[j], mul(W[i], u[j]));
        }
        const uint64_t ch = wt.step(pr, c);
        if (pr.st != ZIGZ_OK) return 0;
        for (unsigned j = 0; j < M; j++) {  // partialEval's MSB-first bind, in place
            std::vector<uint64_t> &t = pool[j];
            for (size_t x = 0; x < half; x++) t[x] = f_add(t[x], mul(ch, f_sub(t[x + half], t[x])));
            t.resize(half);
        }
    }
    if (pr.round != pr.nv) pr.st = ZIGZ_ERR_PROTOCOL_ERROR;  // sumcheck_prover.zig:80-82
    if (pool[0].empty()) return 0;
    uint64_t ev[MAX_TABLES];
    for (unsigned j = 0; j < M; j++) ev[j] = pool[j][0];
    if (table_evals)
        for (unsigned j = 0; j < M; j++) table_evals[j] = ev[j];
    return combine(terms, T, ev);
}
// the sop prover's: pr.ncoef is D + 1
inline uint64_t tail_rounds(SumcheckRounds &pr, std::vector<uint64_t> *pool, unsigned M, const Term *terms, unsigned T,
                            uint64_t *table_evals = nullptr) {
    Unweighted wt;
    return tail_rounds_of(pr, wt, pool, M, terms, T, table_evals);
}

// ------------------------------------------------------------------ verification
// The arguments of zigz_[dev_]sumcheck_verify_sop_batch: the prover's layout; tables holds NULL where the pool entry is eq(tau, .)
// (table_kinds, may be NULL: all tables), whose tau is the next v_i words of eq_points; table_evals may be NULL
struct VerifyArgs {
    size_t k;
    const unsigned *n_tables;
    const void *const *tables;
    const uint8_t *table_kinds;
    const uint64_t *eq_points;
    const size_t *ns;
    const unsigned *n_terms, *term_degrees;
    const uint8_t *term_tables;
    const uint64_t *term_coeffs;
    const uint64_t *claimed_sums, *rounds, *points, *table_evals, *final_evals;
    uint32_t flags;
    const size_t *n_rejected;
};
inline uint8_t kind_of(const VerifyArgs &a, size_t entry) { return a.table_kinds ? a.table_kinds[entry] : pv::KIND_TABLE; }

// The per-proof walk of the verifying entries' checks (these and zerocheck_host.hpp's), over a VerifyArgs `a` of either: ZIGZ_OK,
// or the status of the first proof it rejects, whose index goes to *bad_index.  Per proof, in order: the pool size, the term
// count, the terms; the entries' kinds (entry(e): 1 a table, 0 a closed form, -1 ZIGZ_ERR_INVALID_ARGUMENT); the prover's rule
// over the proof's table entries and its point; then the words of the proof -- D + extra_coef per round --, of its evals, of its
// coefficients and whatever eq_words(i, v, closed forms of the proof) says of the family's taus (ZIGZ_ERR_NOT_CANONICAL).
template <class A, class Entry, class EqWords>
inline zigz_status verify_walk(const A &a, bool dev, bool values, unsigned extra_coef, size_t *bad_index, Entry entry, EqWords eq_words) {
    if (!a.n_rejected || (a.flags & ~(uint32_t)ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED)) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (a.k == 0) return ZIGZ_OK;
    if (a.k > ZIGZ_BATCH_MAX || !a.n_tables || !a.tables || !a.ns || !a.n_terms || !a.term_degrees || !a.term_tables || !a.term_coeffs ||
        !a.claimed_sums || !a.rounds || !a.points || !a.final_evals)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule{dev, values, true, true, sv::SV_MAX_LOG2_N};
    size_t moff = 0, toff = 0, xoff = 0, voff = 0, roff = 0;
    for (size_t i = 0; i < a.k; i++) {
        const unsigned M = a.n_tables[i], T = a.n_terms[i];
        size_t nf = 0;
        zigz_status st = check_terms(M, T, a.term_degrees + toff, a.term_tables + xoff, &nf);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        const void *tables[MAX_TABLES];
        unsigned nt = 0, D = 0;
        for (unsigned j = 0; j < M; j++) {
            const int kind = entry(moff + j);
            if (kind < 0) return fail_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
            if (kind) tables[nt++] = a.tables[moff + j];
        }
        st = table_rule(rule, tables, nt, a.ns[i], a.points + voff);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        for (unsigned t = 0; t < T; t++)
            if (a.term_degrees[toff + t] > D) D = a.term_degrees[toff + t];
        const size_t v = log2_floor(a.ns[i]);
        if (!canonical(a.rounds + roff, (D + extra_coef) * v) || a.claimed_sums[i] >= ZIGZ_BABYBEAR_P || a.final_evals[i] >= ZIGZ_BABYBEAR_P ||
            (a.table_evals && !canonical(a.table_evals + moff, M)) || !canonical(a.term_coeffs + toff, T) || !eq_words(i, v, M - nt))
            return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        moff += M;
        toff += T;
        xoff += nf;
        voff += v;
        roff += (D + extra_coef) * v;
    }
    return ZIGZ_OK;
}
// The host forms' checks in the family's order, from the status `st` of the walk and the proof `bad` it stopped at: a TABLE entry
// (is_table(e)) that holds a value >= p in a proof BEFORE the first one that fails another check is reported instead, with its proof
template <class A, class IsTable>
inline zigz_status verify_walk_host(const A &a, zigz_status st, size_t bad, size_t *bad_index, bool *value_found, IsTable is_table) {
    if (value_found) *value_found = false;
    if (st == ZIGZ_OK || bad >= a.k) return st;
    size_t moff = 0;
    for (size_t i = 0; i < bad; i++)  // (their pool sizes, kinds and pointers have passed)
        for (unsigned j = 0; j < a.n_tables[i]; j++, moff++)
            if (is_table(moff) && !canonical((const uint64_t *)a.tables[moff], a.ns[i])) {
                if (value_found) *value_found = true;
                return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
            }
    return fail_at(bad_index, bad, st);
}

// What zigz_[dev_]sumcheck_verify_sop_batch say about their arguments before anything runs, as pv::check_verify_product_batch:
// verify_walk with D + 1 words per round; a kind is wrong when it is unknown, an eq entry with a table pointer, or an eq entry
// without eq_points; a proof's taus are the next v words of eq_points per eq entry.
inline zigz_status check_verify_sop_batch(const VerifyArgs &a, bool dev, bool values, size_t *bad_index) {
    size_t eoff = 0;
    return verify_walk(
        a, dev, values, 1, bad_index,
        [&](size_t e) {
            const uint8_t kind = kind_of(a, e);
            if (kind == pv::KIND_TABLE) return 1;
            return kind != pv::KIND_EQ || a.tables[e] || !a.eq_points ? -1 : 0;
        },
        [&](size_t, size_t v, unsigned neq) {
            if (neq && !canonical(a.eq_points + eoff, neq * v)) return false;
            eoff += neq * v;
            return true;
        });
}
inline zigz_status check_verify_sop_batch_host(const VerifyArgs &a, size_t *bad_index, bool *value_found = nullptr) {
    size_t bad = a.k;
    const zigz_status st = check_verify_sop_batch(a, false, false, &bad);
    return verify_walk_host(a, st, bad, bad_index, value_found, [&](size_t e) { return kind_of(a, e) == pv::KIND_TABLE; });
}

// the final check once the M pool entries' evaluations are known: their combination equals the last claim and final_eval, and
// (when the proof's table evals are checked) every oracle its table eval
inline uint8_t verdict(const sv::Replay &r, const Term *terms, unsigned T, const uint64_t *oracle_evals, unsigned M, uint64_t final_eval,
                       const uint64_t *table_evals) {
    const uint64_t o = combine(terms, T, oracle_evals);
    bool ok = r.rounds_ok && o == r.expected && o == final_eval;
    if (table_evals)
        for (unsigned j = 0; j < M; j++) ok = ok && oracle_evals[j] == table_evals[j];
    return ok ? 1 : 0;
}

}  // namespace sop
}  // namespace zk
