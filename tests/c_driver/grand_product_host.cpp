// Stand-alone driver of zigz_amd/csrc/grand_product_host.hpp (no GPU, no HIP): built with -fsanitize=address,undefined by
// tests/test_grand_product_cpu.py and run as a child process.
//   prove FILE    FILE holds one instance per line: n fixed, then n column values, then (fixed != 0) v (v + 1) / 2 challenges.  Runs
//                 the prover's argument checker over the whole batch (must pass), builds every tree on the host (gp::build_tree),
//                 walks the layers (gp::Walk, gp::prove_host_layer) and prints one line per proof -- product leaf_eval, the 2 v layer
//                 evals, the 2 v (v - 1) round words, the v (v - 1) / 2 round challenges, the v layer challenges, the v words of the
//                 leaf point.  On the way it checks that every layer's round-0 g(0) + g(1) equals the carried claim (exit status
//                 5) and that the weight's prefix scalar after the last round equals eq(tau, q) (6).  For a Fiat-Shamir proof a
//                 second line holds the verifier's replay and verdict over it: "accept expected oracle".
//   verify FILE   one case per line: n, then n column values, then the proof's words: product, 2 v layer evals, 2 v (v - 1) round
//                 words, v leaf-point words, leaf_eval.  Runs the verifier's argument checker (must pass) and prints "accept expected
//                 oracle" for the column's evaluation as oracle, then the same with the leaf deferred ("accept expected -").
//   check         checks the layout for every v from 1 to ZIGZ_PRODUCT_MAX_LOG2_N (exit status 7), then runs the argument
//                 checkers on bad shapes and prints "case status bad_index" per case (bad_index -1: untouched).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "grand_product_host.hpp"

using namespace zk;

namespace {

const size_t UNTOUCHED = (size_t)-1;
const uint64_t SENTINEL = 0xA5A5A5A5A5A5A5A5ull;

struct Proof {
    uint64_t product = SENTINEL, leaf_eval = SENTINEL;
    std::vector<uint64_t> evals, rounds, points, chs, leaf;
    explicit Proof(size_t v = 0)
        : evals(gp::eval_words(v), SENTINEL), rounds(v ? gp::round_words(v) : 0, SENTINEL), points(v ? gp::point_words(v) : 0, SENTINEL),
          chs(v, SENTINEL), leaf(v, SENTINEL) {}
};

bool read_words(FILE *fp, size_t n, std::vector<uint64_t> &out) {
    out.resize(n);
    for (size_t i = 0; i < n; i++) {
        unsigned long long x;
        if (fscanf(fp, "%llu", &x) != 1) return false;
        out[i] = x;
    }
    return true;
}

void print_words(const std::vector<uint64_t> &w) {
    for (uint64_t x : w) printf(" %llu", (unsigned long long)x);
}

// Multilinear.eval: coordinate 0 with the LSB of the index
uint64_t mle(std::vector<uint64_t> t, const uint64_t *pt) {
    for (size_t j = 0; t.size() > 1; j++) {
        const size_t half = t.size() / 2;
        for (size_t x = 0; x < half; x++) t[x] = f_add(t[2 * x], f_mul(pt[j], f_sub(t[2 * x + 1], t[2 * x])));
        t.resize(half);
    }
    return t[0];
}

int prove(const char *path) {
    FILE *fp = fopen(path, "r");
    if (!fp) return 2;
    std::vector<std::vector<uint64_t>> cols, fixed;
    unsigned long long n, fx;
    while (fscanf(fp, "%llu %llu", &n, &fx) == 2) {
        if (n < 2 || (n & (n - 1)) || n > ((size_t)2 << gp::HOST_LAYER)) return 2;
        std::vector<uint64_t> c, f;
        if (!read_words(fp, n, c) || (fx && !read_words(fp, gp::fixed_words(log2_floor(n)), f))) return 2;
        cols.push_back(c);
        fixed.push_back(f);
    }
    fclose(fp);
    {  // the checker over the batch (the fixed challenges are one flat array: all instances or none)
        std::vector<const void *> tabs;
        std::vector<size_t> ns;
        for (auto &c : cols) {
            tabs.push_back(c.data());
            ns.push_back(c.size());
        }
        uint64_t dummy = 0;
        size_t bad = UNTOUCHED;
        const gp::ProveArgs a{cols.size(), tabs.data(), ns.data(), nullptr, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy};
        if (gp::check_prove_batch(a, false, true, &bad) != ZIGZ_OK) return 1;
    }
    for (size_t i = 0; i < cols.size(); i++) {
        const std::vector<uint64_t> &col = cols[i];
        const size_t nn = col.size(), v = log2_floor(nn);
        std::vector<uint64_t> tree(nn, SENTINEL);
        gp::build_tree(col.data(), nn, tree.data());
        if (tree[nn - 1] != SENTINEL) return 4;
        Proof p(v);
        gp::Walk w;
        w.v = v;
        w.fixed = fixed[i].empty() ? nullptr : fixed[i].data();
        w.product = &p.product;
        w.layer_evals = p.evals.data();
        w.rounds = p.rounds.data();
        w.points = p.points.data();
        w.layer_challenges = p.chs.data();
        w.leaf_point = p.leaf.data();
        w.leaf_eval = &p.leaf_eval;
        w.begin(tree[gp::layer_at(nn, 0)]);
        for (size_t j = 0; j < v; j++) {
            const uint64_t *next = j + 1 == v ? col.data() : tree.data() + gp::layer_at(nn, (unsigned)(j + 1));
            const uint64_t carried = w.claim;
            const std::vector<uint64_t> tau = w.tau;
            uint64_t prefix = SENTINEL;
            gp::prove_host_layer(w, j, next, &prefix);
            if (w.st != ZIGZ_OK) return 3;
            if (j && w.layer_claim != carried) return 5;
            std::vector<uint64_t> q(j);
            for (size_t x = 0; x < j; x++) q[x] = p.points[gp::points_at(j) + j - 1 - x];
            if (prefix != pv::eq_at(tau.data(), q.data(), j)) return 6;
        }
        w.finish();
        printf("%llu %llu", (unsigned long long)p.product, (unsigned long long)p.leaf_eval);
        print_words(p.evals);
        print_words(p.rounds);
        print_words(p.points);
        print_words(p.chs);
        print_words(p.leaf);
        printf("\n");
        if (fixed[i].empty()) {
            const gp::Replay rep = gp::replay(p.product, p.evals.data(), p.rounds.data(), v);
            const uint64_t oracle = mle(col, p.leaf.data());
            printf("%d %llu %llu\n", (int)gp::verdict(rep, p.leaf.data(), v, p.leaf_eval, &oracle), (unsigned long long)rep.expected,
                   (unsigned long long)oracle);
        }
    }
    return 0;
}

int verify(const char *path) {
    FILE *fp = fopen(path, "r");
    if (!fp) return 2;
    unsigned long long n;
    while (fscanf(fp, "%llu", &n) == 1) {
        if (n < 2 || (n & (n - 1))) return 2;
        const size_t v = log2_floor(n);
        std::vector<uint64_t> col, product, evals, rounds, leaf, le;
        if (!read_words(fp, n, col) || !read_words(fp, 1, product) || !read_words(fp, gp::eval_words(v), evals) ||
            !read_words(fp, gp::round_words(v), rounds) || !read_words(fp, v, leaf) || !read_words(fp, 1, le))
            return 2;
        const void *tab = col.data();
        const size_t nn = n;
        size_t bad = UNTOUCHED, rejected = 0;
        const gp::VerifyArgs a{1, &tab, &nn, product.data(), evals.data(), rounds.data(), leaf.data(), le.data(), 0, &rejected};
        if (gp::check_verify_batch(a, false, true, &bad) != ZIGZ_OK) return 1;
        const gp::Replay rep = gp::replay(product[0], evals.data(), rounds.data(), v);
        const uint64_t oracle = mle(col, leaf.data());
        printf("%d %llu %llu\n", (int)gp::verdict(rep, leaf.data(), v, le[0], &oracle), (unsigned long long)rep.expected,
               (unsigned long long)oracle);
        printf("%d %llu -\n", (int)gp::verdict(rep, leaf.data(), v, le[0], nullptr), (unsigned long long)rep.expected);
    }
    fclose(fp);
    return 0;
}

// ---- the layout: for every v the layers lie inside the n words, one behind the other from the top down, none reaches word n - 1,
// every layer of 4 words or more is 16-byte aligned; the passes end at a layer k_gp_top takes; the outputs' offsets add up
bool layout_ok() {
    for (unsigned v = 1; v <= ZIGZ_PRODUCT_MAX_LOG2_N; v++) {
        const size_t n = (size_t)1 << v;
        size_t expect = 0;
        for (unsigned j = v; j-- > 0;) {
            const size_t at = gp::layer_at(n, j), len = (size_t)1 << j;
            if (at != expect || at + len > n - 1 || (len >= 4 && at % 4)) {
                fprintf(stderr, "v %u: layer %u at word %zu (%zu words), expected at %zu\n", v, j, at, len, expect);
                return false;
            }
            expect = at + len;
        }
        if (expect != n - 1) return false;
        unsigned J = v, passes = 0;
        for (unsigned lv; (lv = gp::fused_levels(J)) != 0; J -= lv, passes++)
            if (lv > gp::MAX_FUSED || J - lv < gp::TOP_LOG2) return false;
        if (J > gp::TOP_LOG2 || (v > gp::TOP_LOG2 && (J != gp::TOP_LOG2 || passes != (v - gp::TOP_LOG2 + 2) / 3))) return false;
        size_t r = 0, p = 0;
        for (size_t j = 0; j < v; j++) {
            if (gp::rounds_at(j) != r || gp::points_at(j) != p || gp::fixed_at(j) != p + j) return false;
            r += 4 * j;
            p += j;
        }
        if (gp::round_words(v) != r || gp::point_words(v) != p || gp::fixed_words(v) != p + v || gp::eval_words(v) != 2 * v) return false;
    }
    const size_t big[2] = {(size_t)1 << 30, 2048};
    return gp::first_pass_chunks(big, 2) == ((size_t)1 << 17);
}

struct Batch {  // three instances: 8, 4 and 16 words
    std::vector<size_t> ns{8, 4, 16};
    alignas(16) uint64_t col[3][16];
    alignas(16) uint64_t outbuf[3][16];
    std::vector<const void *> tables, out;
    std::vector<uint64_t> fixed;  // 6 + 3 + 10 words
    const uint64_t *fixed_p = nullptr;
    // the proof words of the verifier's cases: canonical zeros; 2 v = 6, 4, 8 eval words, 2 v (v - 1) = 12, 4, 24 round words
    uint64_t products[3] = {}, evals[18] = {}, rounds[40] = {}, points[16] = {}, chs[9] = {}, leafs[9] = {}, les[3] = {};
    const void *a_tables, *a_ns, *a_out;
    void *a_products, *a_evals, *a_rounds, *a_points, *a_chs, *a_leafs, *a_les;
    size_t k = 3;
    Batch() {
        for (auto &c : col)
            for (size_t i = 0; i < 16; i++) c[i] = (7654321 * (i + 1) + (size_t)(&c - col)) % ZIGZ_BABYBEAR_P;
        for (auto &c : col) tables.push_back(c);
        for (auto &o : outbuf) out.push_back(o);
        fixed.assign(6 + 3 + 10, 5);
        a_tables = tables.data();
        a_ns = ns.data();
        a_out = out.data();
        a_products = products;
        a_evals = evals;
        a_rounds = rounds;
        a_points = points;
        a_chs = chs;
        a_leafs = leafs;
        a_les = les;
    }
};

void layers_case(const char *name, Batch &b, bool dev) {
    size_t bad = UNTOUCHED;
    const gp::LayersArgs a{b.k, (const void *const *)b.a_tables, (const size_t *)b.a_ns, (const void *const *)b.a_out};
    zigz_status st = gp::check_layers_batch(a, dev, false, &bad);
    if (!dev && st == ZIGZ_OK) st = gp::check_layers_batch(a, false, true, &bad);  // (the library finds a value >= p while it narrows)
    printf("layers_%s_%s %d %lld\n", name, dev ? "dev" : "host", (int)st, (long long)bad);
}

void prove_case(const char *name, Batch &b, bool dev) {
    size_t bad = UNTOUCHED;
    const gp::ProveArgs a{b.k,        (const void *const *)b.a_tables, (const size_t *)b.a_ns, b.fixed_p, b.a_products, b.a_evals, b.a_rounds,
                          b.a_points, b.a_chs,                         b.a_leafs,              b.a_les};
    zigz_status st;
    if (dev) {
        st = gp::check_prove_batch(a, true, false, &bad);
    } else {  // the host form's order: a column's value >= p in front of the first instance that fails another check is reported instead
        st = checks_in_call_order((const uint64_t *const *)b.tables.data(), b.ns.data(), b.k, &bad,
                                  [&](size_t *f) { return gp::check_prove_batch(a, false, false, f); });
        if (st == ZIGZ_OK) st = gp::check_prove_batch(a, false, true, &bad);
    }
    printf("prove_%s_%s %d %lld\n", name, dev ? "dev" : "host", (int)st, (long long)bad);
}

void verify_case(const char *name, Batch &b, uint32_t flags, bool no_tables = false, bool no_rejected = false) {
    for (int dev = 0; dev < 2; dev++) {
        size_t bad = UNTOUCHED, rejected = 0;
        const gp::VerifyArgs a{b.k,
                               no_tables ? nullptr : (const void *const *)b.a_tables,
                               (const size_t *)b.a_ns,
                               (const uint64_t *)b.a_products,
                               (const uint64_t *)b.a_evals,
                               (const uint64_t *)b.a_rounds,
                               (const uint64_t *)b.a_leafs,
                               (const uint64_t *)b.a_les,
                               flags,
                               no_rejected ? nullptr : &rejected};
        const zigz_status st = gp::check_verify_batch(a, dev != 0, false, &bad);
        printf("verify_%s_%s %d %lld\n", name, dev ? "dev" : "host", (int)st, (long long)bad);
    }
}

int check() {
    if (!layout_ok()) return 7;
    const uint64_t p = ZIGZ_BABYBEAR_P;
    for (int dev = 0; dev < 2; dev++) {
        { Batch b; layers_case("ok", b, dev); }
        { Batch b; b.k = 0; b.a_out = nullptr; layers_case("k0", b, dev); }
        { Batch b; b.k = ZIGZ_BATCH_MAX + 1; layers_case("k4097", b, dev); }
        { Batch b; b.a_out = nullptr; layers_case("no_out", b, dev); }
        { Batch b; b.a_ns = nullptr; layers_case("no_ns", b, dev); }
        { Batch b; b.tables[1] = nullptr; layers_case("null_column_1", b, dev); }
        { Batch b; b.out[2] = nullptr; layers_case("null_out_2", b, dev); }
        { Batch b; b.ns[0] = 0; layers_case("n0_0", b, dev); }
        { Batch b; b.ns[1] = 1; layers_case("n1_1", b, dev); }
        { Batch b; b.ns[2] = 12; layers_case("n12_2", b, dev); }
        { Batch b; b.ns[2] = (size_t)1 << 31; layers_case("n2p31_2", b, dev); }
        { Batch b; b.ns[1] = 3; b.out[0] = nullptr; layers_case("null_out_0_before_n3_1", b, dev); }
        { Batch b; prove_case("ok", b, dev); }
        { Batch b; b.fixed_p = b.fixed.data(); prove_case("ok_fixed", b, dev); }
        { Batch b; b.k = 0; b.a_products = nullptr; prove_case("k0", b, dev); }
        { Batch b; b.k = ZIGZ_BATCH_MAX + 1; prove_case("k4097", b, dev); }
        { Batch b; b.a_products = nullptr; prove_case("no_products", b, dev); }
        { Batch b; b.a_rounds = nullptr; prove_case("no_rounds", b, dev); }
        { Batch b; b.a_leafs = nullptr; prove_case("no_leaf_points", b, dev); }
        { Batch b; b.tables[2] = nullptr; prove_case("null_column_2", b, dev); }
        { Batch b; b.ns[0] = 0; prove_case("n0_0", b, dev); }
        { Batch b; b.ns[1] = 1; prove_case("n1_1", b, dev); }
        { Batch b; b.ns[1] = 3; prove_case("n3_1", b, dev); }
        { Batch b; b.ns[2] = (size_t)1 << 31; prove_case("n2p31_2", b, dev); }
        // the fixed challenges: 6 words, then 3, then 10; a word >= p in every instance's last place, and the first failing instance wins
        { Batch b; b.fixed[5] = p; b.fixed_p = b.fixed.data(); prove_case("challenge_0_last", b, dev); }
        { Batch b; b.fixed[8] = p; b.fixed_p = b.fixed.data(); prove_case("challenge_1_last", b, dev); }
        { Batch b; b.fixed[18] = ~(uint64_t)0; b.fixed_p = b.fixed.data(); prove_case("challenge_2_last", b, dev); }
        { Batch b; b.fixed[6] = p; b.ns[2] = 12; b.fixed_p = b.fixed.data(); prove_case("challenge_1_before_n12_2", b, dev); }
        { Batch b; b.fixed[9] = p; b.ns[1] = 3; b.fixed_p = b.fixed.data(); prove_case("n3_1_before_challenge_2", b, dev); }
    }
    { Batch b; b.tables[1] = (const uint8_t *)b.col[1] + 8; layers_case("misaligned_column_1", b, true); }
    { Batch b; b.out[1] = (const uint8_t *)b.outbuf[1] + 4; layers_case("misaligned_out_1", b, true); }
    { Batch b; b.tables[2] = (const uint8_t *)b.col[2] + 8; prove_case("misaligned_2", b, true); }
    { Batch b; b.col[1][3] = p; layers_case("value_1", b, false); }
    { Batch b; b.col[2][15] = p; prove_case("value_2", b, false); }
    { Batch b; b.col[0][7] = p; b.ns[1] = 3; prove_case("value_0_before_n3_1", b, false); }
    { Batch b; b.col[2][0] = p; b.ns[1] = 3; prove_case("n3_1_before_value_2", b, false); }
    // the verifier's checker
    { Batch b; verify_case("ok", b, 0); }
    { Batch b; verify_case("ok_deferred", b, ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED, true); }
    { Batch b; verify_case("deferred_with_columns", b, ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED); }
    { Batch b; verify_case("no_columns", b, 0, true); }
    { Batch b; verify_case("flags2", b, 2); }
    { Batch b; verify_case("no_n_rejected", b, 0, false, true); }
    { Batch b; b.k = 0; b.a_products = nullptr; verify_case("k0", b, 0); }
    { Batch b; b.a_evals = nullptr; verify_case("no_layer_evals", b, 0); }
    { Batch b; b.a_les = nullptr; verify_case("no_leaf_evals", b, 0); }
    { Batch b; b.ns[1] = 1; verify_case("n1_1", b, 0); }
    { Batch b; b.ns[1] = 1; verify_case("deferred_n1_1", b, ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED, true); }
    { Batch b; b.ns[2] = 12; verify_case("deferred_n12_2", b, ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED, true); }
    { Batch b; b.products[1] = p; verify_case("product_1", b, 0); }
    { Batch b; b.evals[5] = p; verify_case("layer_eval_0_last", b, 0); }
    { Batch b; b.evals[9] = p; verify_case("layer_eval_1_last", b, 0); }
    { Batch b; b.rounds[11] = p; verify_case("round_word_0_last", b, 0); }
    { Batch b; b.rounds[15] = p; verify_case("round_word_1_last", b, 0); }
    { Batch b; b.rounds[39] = p; verify_case("round_word_2_last", b, 0); }
    { Batch b; b.leafs[4] = p; verify_case("leaf_point_1_last", b, 0); }
    { Batch b; b.les[2] = p; verify_case("leaf_eval_2", b, ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED, true); }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "prove")) return prove(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "verify")) return verify(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    fprintf(stderr, "usage: grand_product_host prove FILE | verify FILE | check\n");
    return 2;
}
