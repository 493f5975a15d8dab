#pragma once
// The host side of the batched grand-product argument (api_grand_product.cpp, grand_product.hip): instance i is a
// column A of n = 2^v canonical words and proves prod_x A[x] through the layered product tree
//   V_v = A,   V_j[x] = V_{j+1}[x] V_{j+1}[x + 2^j]  (x < 2^j),   L_j = V_{j+1}[0 : 2^j],  H_j = V_{j+1}[2^j : 2^(j+1)],
// the HALVES pairing: it matches the MSB-first bind, and the two operands of a layer are contiguous sub-arrays.  Layer 0 hands
// over l_0 = V_1[0], h_0 = V_1[1]; layer j >= 1 is the closed-form zero-check (zerocheck_host.hpp) of sum_x eq(tau^(j), x) L_j(x)
// H_j(x) = claim_j -- j rounds of 4 coefficients --, after which l_j = L_j(q), h_j = H_j(q) at q = the round challenges reversed,
// c_j is drawn, tau^(j+1) = (q, c_j) and claim_(j+1) = l_j + c_j (h_j - l_j).  ONE transcript per instance runs through all
// layers: it absorbs the product, then per layer the rounds as SumcheckRounds::step absorbs them, then l_j, h_j.  Points are in
// Multilinear.eval's convention throughout (coordinate 0 goes with the LSB of the index).
// Here: where a layer lives in a tree buffer and where a layer's words live in the outputs, the argument rules of the six
// entries, the walk through the layers (Walk), the prover of a layer whose tables are small enough for the host, and the
// verifier's replay and verdict.  On top of zerocheck_host.hpp.  Plain C++, no HIP: testable without a GPU
// (tests/c_driver/grand_product_host.cpp).
#include "zerocheck_host.hpp"

namespace zk {
namespace gp {

constexpr unsigned TOP_LOG2 = 11;    // k_gp_top takes a tree from its first layer of at most 2^11 words down to layer 0
constexpr unsigned HOST_LAYER = 10;  // the layers j <= 10 (tables of at most 1024 words) are proved on the host
constexpr unsigned MAX_FUSED = 3;    // levels one pass of k_gp_layers computes
static_assert(((size_t)1 << HOST_LAYER) == HOST_TAIL_MAX && TOP_LOG2 == HOST_LAYER + 1, "the top hand-off holds V_11: L_10 and H_10");

// ---- layout.  A tree buffer of an instance of n = 2^v words holds the layers v - 1 .. 0, layer j (2^j words) at word
// n - 2^(j+1): every layer of 4 words or more is 16-byte aligned, word n - 1 is unused.
inline size_t layer_at(size_t n, unsigned j) { return n - ((size_t)2 << j); }
// the levels the pass that starts at layer J computes (0: the rest is k_gp_top's)
inline unsigned fused_levels(unsigned J) { return J <= TOP_LOG2 ? 0 : J - TOP_LOG2 < MAX_FUSED ? J - TOP_LOG2 : MAX_FUSED; }
// One launch serves all columns: a grid holds fewer than 2^32 threads, i.e. fewer than 2^24 workgroups of 256.  The first pass is
// the largest: a column longer than 2048 words in chunks of 8192 words (and a layer's zero-check reads tables half as long).
constexpr size_t CHUNK = 8192, MAX_CHUNKS = ((size_t)1 << 24) - 1;
inline size_t first_pass_chunks(const size_t *ns, size_t k) {
    size_t c = 0;
    for (size_t i = 0; i < k; i++)
        if (ns[i] > ((size_t)1 << TOP_LOG2)) c += (ns[i] + CHUNK - 1) / CHUNK;
    return c;
}
// an instance's words in the flat outputs, and where layer j's words start among them (layer 0 has no rounds)
inline size_t eval_words(size_t v) { return 2 * v; }
inline size_t round_words(size_t v) { return 2 * v * (v - 1); }
inline size_t point_words(size_t v) { return v * (v - 1) / 2; }
inline size_t fixed_words(size_t v) { return v * (v + 1) / 2; }
inline size_t rounds_at(size_t j) { return j ? 2 * j * (j - 1) : 0; }
inline size_t points_at(size_t j) { return j ? j * (j - 1) / 2 : 0; }
inline size_t fixed_at(size_t j) { return j * (j + 1) / 2; }  // layer j's round challenges in order of use; c_j follows them

// the tree of a host column, in the layout above (tree: n words, the last one untouched)
inline void build_tree(const uint64_t *col, size_t n, uint64_t *tree) {
    const uint64_t *src = col;
    for (unsigned j = log2_floor(n); j-- > 0;) {
        uint64_t *dst = tree + layer_at(n, j);
        for (size_t x = 0; x < ((size_t)1 << j); x++) dst[x] = f_mul(src[x], src[x + ((size_t)1 << j)]);
        src = dst;
    }
}

// ---- the arguments
// zigz_[dev_]product_layers_batch
struct LayersArgs {
    size_t k;
    const void *const *tables;
    const size_t *ns;
    const void *const *out;
};
// zigz_[dev_]grand_product_prove_batch
struct ProveArgs {
    size_t k;
    const void *const *tables;
    const size_t *ns;
    const uint64_t *fixed;
    const void *products, *layer_evals, *rounds, *points, *layer_challenges, *leaf_points, *leaf_evals;
};
// zigz_[dev_]grand_product_verify_batch
struct VerifyArgs {
    size_t k;
    const void *const *tables;
    const size_t *ns;
    const uint64_t *products, *layer_evals, *rounds, *leaf_points, *leaf_evals;
    uint32_t flags;
    const size_t *n_rejected;
};

// the family's rule for one column: a NULL device pointer, the shape, the length, n = 1, the pointer and its alignment, the values
inline TableRule column_rule(bool dev, bool values) { return TableRule{dev, values, true, false, ZIGZ_PRODUCT_MAX_LOG2_N}; }

// What the entries say about their arguments before anything runs: ZIGZ_OK, or the status of the first instance they reject, whose
// index goes to *bad_index.  Per instance, in order: the column (column_rule), then the output buffer (NULL, or on the device not
// 16-byte aligned: ZIGZ_ERR_INVALID_ARGUMENT).  k == 0 is ZIGZ_OK.
inline zigz_status check_layers_batch(const LayersArgs &a, bool dev, bool values, size_t *bad_index) {
    if (a.k == 0) return ZIGZ_OK;
    if (a.k > ZIGZ_BATCH_MAX || !a.tables || !a.ns || !a.out) return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule = column_rule(dev, values);
    for (size_t i = 0; i < a.k; i++) {
        const zigz_status st = table_rule(rule, a.tables + i, 1, a.ns[i], nullptr);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        if (!a.out[i] || (dev && ((uintptr_t)a.out[i] & 15))) return fail_at(bad_index, i, ZIGZ_ERR_INVALID_ARGUMENT);
    }
    return ZIGZ_OK;
}

// ... the prover's: the column, then the instance's v (v + 1) / 2 fixed challenges (a word >= p: ZIGZ_ERR_NOT_CANONICAL); an
// output array NULL is ZIGZ_ERR_INVALID_ARGUMENT
inline zigz_status check_prove_batch(const ProveArgs &a, bool dev, bool values, size_t *bad_index) {
    if (a.k == 0) return ZIGZ_OK;
    if (a.k > ZIGZ_BATCH_MAX || !a.tables || !a.ns || !a.products || !a.layer_evals || !a.rounds || !a.points || !a.layer_challenges ||
        !a.leaf_points || !a.leaf_evals)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule = column_rule(dev, values);
    size_t foff = 0;
    for (size_t i = 0; i < a.k; i++) {
        const zigz_status st = table_rule(rule, a.tables + i, 1, a.ns[i], nullptr);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        const size_t w = fixed_words(log2_floor(a.ns[i]));
        if (a.fixed && !canonical(a.fixed + foff, w)) return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        foff += w;
    }
    return ZIGZ_OK;
}

// ... the verifier's.  In front of the proofs: n_rejected NULL, an unknown flag, a NULL input array, and the columns -- required
// without ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED, forbidden with it (ZIGZ_ERR_INVALID_ARGUMENT).  Per proof: the column (deferred: the
// shape and the length alone), then the words of the proof (ZIGZ_ERR_NOT_CANONICAL).
inline zigz_status check_verify_batch(const VerifyArgs &a, bool dev, bool values, size_t *bad_index) {
    if (!a.n_rejected || (a.flags & ~(uint32_t)ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED)) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (a.k == 0) return ZIGZ_OK;
    const bool deferred = (a.flags & ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED) != 0;
    if (a.k > ZIGZ_BATCH_MAX || !a.ns || !a.products || !a.layer_evals || !a.rounds || !a.leaf_points || !a.leaf_evals ||
        deferred != (a.tables == nullptr))
        return ZIGZ_ERR_INVALID_ARGUMENT;
    const TableRule rule = column_rule(dev, values);
    size_t eoff = 0, roff = 0, voff = 0;
    for (size_t i = 0; i < a.k; i++) {
        zigz_status st;
        if (deferred) {
            st = mle_check(a.ns[i]);
            if (st == ZIGZ_OK && log2_floor(a.ns[i]) > ZIGZ_PRODUCT_MAX_LOG2_N) st = ZIGZ_ERR_INVALID_ARGUMENT;
            if (st == ZIGZ_OK && a.ns[i] == 1) st = ZIGZ_ERR_NO_VARIABLES;
        } else {
            st = table_rule(rule, a.tables + i, 1, a.ns[i], nullptr);
        }
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        const size_t v = log2_floor(a.ns[i]);
        if (a.products[i] >= ZIGZ_BABYBEAR_P || !canonical(a.layer_evals + eoff, eval_words(v)) || !canonical(a.rounds + roff, round_words(v)) ||
            !canonical(a.leaf_points + voff, v) || a.leaf_evals[i] >= ZIGZ_BABYBEAR_P)
            return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        eoff += eval_words(v);
        roff += round_words(v);
        voff += v;
    }
    return ZIGZ_OK;
}

// ---- the prover's walk through the layers of ONE instance: its transcript, the carried claim and tau, and its outputs
struct Walk {
    size_t v = 0;
    const uint64_t *fixed = nullptr;  // the instance's v (v + 1) / 2 challenges in order of use, or none: drawn from the transcript
    uint64_t *product = nullptr, *layer_evals = nullptr, *rounds = nullptr, *points = nullptr, *layer_challenges = nullptr,
             *leaf_point = nullptr, *leaf_eval = nullptr;
    Transcript tr;              // fresh per instance; runs through all layers
    std::vector<uint64_t> tau;  // tau^(j) of the layer that comes next
    uint64_t claim = 0;         // claim_j of the layer that comes next
    uint64_t layer_claim = 0;   // what the layer's round 0 sums to (g(0) + g(1)): the carried claim, for an honest tree
    zigz_status st = ZIGZ_OK;

    void begin(uint64_t prod) {
        *product = prod;
        if (!fixed) tr.append_field(prod);
        claim = prod;
    }
    // the round state of layer j >= 1: 4 coefficients per round, j rounds, the walk's transcript
    SumcheckRounds layer_rounds(size_t j) {
        SumcheckRounds pr;
        pr.ncoef = 4;
        pr.nv = j;
        pr.rounds = rounds + rounds_at(j);
        pr.point = points + points_at(j);
        pr.claimed_sum = &layer_claim;
        pr.fixed = fixed ? fixed + fixed_at(j) : nullptr;
        pr.tr = tr;
        return pr;
    }
    // layer j is through its rounds (pr; layer 0: none) with l = L_j(q), h = H_j(q): records them, draws c_j, carries tau and the claim on
    void close_layer(size_t j, const SumcheckRounds *pr, uint64_t l, uint64_t h) {
        if (pr) {
            tr = pr->tr;
            if (pr->st != ZIGZ_OK) st = pr->st;
        }
        if (st != ZIGZ_OK) return;
        layer_evals[2 * j] = l;
        layer_evals[2 * j + 1] = h;
        uint64_t c;
        if (fixed) {
            c = fixed[fixed_at(j) + j];
            if (c >= ZIGZ_BABYBEAR_P) {
                st = ZIGZ_ERR_NOT_CANONICAL;
                return;
            }
        } else {
            tr.append_field(l);
            tr.append_field(h);
            c = tr.challenge();
        }
        layer_challenges[j] = c;
        tau.resize(j + 1);
        for (size_t x = 0; x < j; x++) tau[x] = points[points_at(j) + j - 1 - x];  // q: the round challenges reversed
        tau[j] = c;
        claim = f_add(l, f_mul(c, f_sub(h, l)));
    }
    void finish() {
        if (st != ZIGZ_OK) return;
        for (size_t x = 0; x < v; x++) leaf_point[x] = tau[x];
        *leaf_eval = claim;
    }
};

// the one term of a layer's zero-check: L * H over the pool (L, H)
inline sop::Term layer_term() {
    sop::Term t{};
    t.alpha = 1;
    t.d = 2;
    t.idx[0] = 0;
    t.idx[1] = 1;
    return t;
}

// Layer j <= HOST_LAYER on the host from V_(j+1) (2^(j+1) canonical words of any unsigned type): layer 0 hands over V_1's two
// words; layer j >= 1 runs zc::tail_rounds over (L_j, H_j) under tau^(j).  *prefix (when asked for): the weight's prefix scalar after
// the last round, which is eq(tau^(j), q)
template <class W>
inline void prove_host_layer(Walk &w, size_t j, const W *next, uint64_t *prefix = nullptr) {
    if (w.st != ZIGZ_OK) return;
    if (j == 0) {
        if (prefix) *prefix = 1;
        w.close_layer(0, nullptr, next[0], next[1]);
        return;
    }
    const size_t m = (size_t)1 << j;
    std::vector<uint64_t> pool[2] = {std::vector<uint64_t>(next, next + m), std::vector<uint64_t>(next + m, next + 2 * m)};
    SumcheckRounds pr = w.layer_rounds(j);
    zc::Weight wt;
    wt.tau = w.tau.data();
    wt.v = j;
    const sop::Term term = layer_term();
    uint64_t lh[2] = {0, 0};
    zc::tail_rounds(pr, wt, pool, 2, &term, 1, 2, lh);
    if (prefix) *prefix = wt.P;
    w.close_layer(j, &pr, lh[0], lh[1]);
}

// ---- verification.  The replay of one proof (Fiat-Shamir): l_0 h_0 == product; per layer j >= 1 the claim chain at 4
// coefficients per round (g(0) + g(1) == claim, absorb, draw, claim = g(challenge)) and eq(tau^(j), q) l_j h_j == the last claim;
// every challenge is derived here.  expected: the claim at the failing step, or claim_v; leaf_point: tau^(v) (when the layers held).
struct Replay {
    bool layers_ok = false;
    uint64_t expected = 0;
    std::vector<uint64_t> leaf_point;
};
inline Replay replay(uint64_t product, const uint64_t *layer_evals, const uint64_t *rounds, size_t v) {
    Replay out;
    Transcript tr;
    tr.append_field(product);
    uint64_t claim = product;
    std::vector<uint64_t> tau, q;
    for (size_t j = 0; j < v; j++) {
        const uint64_t l = layer_evals[2 * j], h = layer_evals[2 * j + 1];
        q.assign(j, 0);
        const uint64_t *r = rounds + rounds_at(j);
        for (size_t x = 0; x < j; x++) {
            const uint64_t *c = r + 4 * x;
            uint64_t s = c[0];
            for (unsigned y = 0; y < 4; y++) s = f_add(s, c[y]);
            if (s != claim) {
                out.expected = claim;
                return out;
            }
            const uint64_t ch = absorb_and_draw(tr, c, 4);
            claim = c[3];
            for (unsigned y = 3; y > 0; y--) claim = f_add(f_mul(claim, ch), c[y - 1]);
            q[j - 1 - x] = ch;
        }
        if (f_mul(pv::eq_at(tau.data(), q.data(), j), f_mul(l, h)) != claim) {  // (layer 0: l_0 h_0 == product)
            out.expected = claim;
            return out;
        }
        tr.append_field(l);
        tr.append_field(h);
        const uint64_t c = tr.challenge();
        tau = q;
        tau.push_back(c);
        claim = f_add(l, f_mul(c, f_sub(h, l)));
    }
    out.layers_ok = true;
    out.expected = claim;
    out.leaf_point.swap(tau);
    return out;
}
// the final check: the layers held, the derived leaf point is the proof's, leaf_eval is claim_v and (oracle != NULL: the column is
// at hand) so is the column's evaluation at the proof's leaf point
inline uint8_t verdict(const Replay &r, const uint64_t *leaf_point, size_t v, uint64_t leaf_eval, const uint64_t *oracle) {
    bool ok = r.layers_ok && leaf_eval == r.expected;
    for (size_t x = 0; ok && x < v; x++) ok = r.leaf_point[x] == leaf_point[x];
    if (oracle) ok = ok && *oracle == r.expected;
    return ok ? 1 : 0;
}

}  // namespace gp
}  // namespace zk
