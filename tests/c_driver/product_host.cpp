// Stand-alone driver of zigz_amd/csrc/product_host.hpp and the rounds of sumcheck_host.hpp under it (no GPU, no HIP): built with
// -fsanitize=address,undefined by tests/test_sumcheck_product_cpu.py and run as a child process.
//   prove FILE   FILE holds one instance per line: d n fixed, then d * n table values, then (fixed != 0) log2 n challenges.  Runs
//                the argument checker over the whole batch (must pass), then proves every instance twice and prints one line per
//                proof -- claimed_sum final_eval, the (d + 1) v round coefficients, the v challenges, the d factor evaluations:
//                  first with the host's own rounds (tail_rounds, what the library runs once a table is <= 1024 long),
//                  then with every round's coefficients assembled (coefficients()) from sums formed the way the kernels form
//                  them: raw 64-bit products added as low and high halves, reduced twice per 16 index pairs, i.e. carrying R^-d.
//   check        runs the argument checkers on bad shapes and prints "case status bad_index written" per case (bad_index -1:
//                untouched; written: 1 if any output word changed).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "field.hpp"
#include "product_host.hpp"

using namespace zk;

namespace {

const size_t UNTOUCHED = (size_t)-1;
const uint64_t SENTINEL = 0xA5A5A5A5A5A5A5A5ull;

struct Instance {
    unsigned d = 0;
    size_t n = 0;
    std::vector<uint64_t> f[pd::MAX_DEGREE];
    std::vector<uint64_t> fixed;
};

bool read_instances(const char *path, std::vector<Instance> &out) {
    FILE *fp = fopen(path, "r");
    if (!fp) return false;
    unsigned long long d, n, fixed, x;
    bool ok = true;
    while (ok && fscanf(fp, "%llu %llu %llu", &d, &n, &fixed) == 3) {
        if (d < 1 || d > pd::MAX_DEGREE || n < 2 || n > HOST_TAIL_MAX || (n & (n - 1))) { ok = false; break; }
        Instance I;
        I.d = (unsigned)d;
        I.n = (size_t)n;
        for (unsigned j = 0; j < I.d && ok; j++)
            for (size_t i = 0; i < I.n && ok; i++) {
                ok = fscanf(fp, "%llu", &x) == 1;
                I.f[j].push_back(x);
            }
        for (size_t r = 0; fixed && ok && r < log2_floor(I.n); r++) {
            ok = fscanf(fp, "%llu", &x) == 1;
            I.fixed.push_back(x);
        }
        if (ok) out.push_back(std::move(I));
    }
    fclose(fp);
    return ok;
}

struct Proof {
    uint64_t claimed = SENTINEL, fe = SENTINEL;
    std::vector<uint64_t> rounds, point, evals;
};

void print_proof(const Proof &p) {
    printf("%llu %llu", (unsigned long long)p.claimed, (unsigned long long)p.fe);
    for (uint64_t x : p.rounds) printf(" %llu", (unsigned long long)x);
    for (uint64_t x : p.point) printf(" %llu", (unsigned long long)x);
    for (uint64_t x : p.evals) printf(" %llu", (unsigned long long)x);
    printf("\n");
}

SumcheckRounds make_prover(const Instance &I, Proof &p) {
    const size_t v = log2_floor(I.n);
    p.rounds.assign((I.d + 1) * v, SENTINEL);
    p.point.assign(v, SENTINEL);
    p.evals.assign(I.d, SENTINEL);
    SumcheckRounds pr;
    pr.ncoef = I.d + 1;
    pr.nv = v;
    pr.claimed_sum = &p.claimed;
    pr.rounds = p.rounds.data();
    pr.point = p.point.data();
    pr.fixed = I.fixed.empty() ? nullptr : I.fixed.data();
    return pr;
}

// the d + 1 sums of one round as sumcheck_product.hip forms them (pd_terms / pd_store): per group of 16 index pairs the raw
// 64-bit products added as low and high halves and reduced twice, the groups' canonical values added and reduced mod p once
void kernel_sums(unsigned d, const std::vector<uint64_t> *f, size_t m, uint64_t *sums) {
    const size_t half = m / 2;
    uint64_t total[pd::MAX_DEGREE + 1] = {0, 0, 0, 0};
    for (size_t g0 = 0; g0 < half; g0 += 16) {
        uint64_t lo[pd::MAX_DEGREE + 1] = {0, 0, 0, 0}, hi[pd::MAX_DEGREE + 1] = {0, 0, 0, 0};
        auto add = [&](unsigned c, uint32_t x, uint32_t y) {
            const uint64_t pr = (uint64_t)x * y;
            lo[c] += (uint32_t)pr;
            hi[c] += pr >> 32;
        };
        for (size_t i = g0; i < g0 + 16 && i < half; i++) {
            uint32_t a[pd::MAX_DEGREE], e[pd::MAX_DEGREE];
            for (unsigned j = 0; j < d; j++) {
                a[j] = (uint32_t)f[j][i];
                e[j] = sub_mod((uint32_t)f[j][i + half], a[j]);
            }
            if (d == 1) {
                lo[0] += a[0];
                lo[1] += e[0];
            } else if (d == 2) {
                add(0, a[0], a[1]);
                add(1, a[0], e[1]);
                add(1, e[0], a[1]);
                add(2, e[0], e[1]);
            } else {
                const uint32_t p = mont_mul(a[0], a[1]), q = mont_mul(e[0], e[1]);
                const uint32_t x = monty_reduce((uint64_t)a[0] * e[1] + (uint64_t)e[0] * a[1]);
                add(0, p, a[2]);
                add(1, p, e[2]);
                add(1, x, a[2]);
                add(2, x, e[2]);
                add(2, q, a[2]);
                add(3, q, e[2]);
            }
        }
        for (unsigned c = 0; c <= d; c++) total[c] += d == 1 ? lo[c] : (uint64_t)monty_reduce(hi[c] + monty_reduce(lo[c]));
    }
    for (unsigned c = 0; c <= d; c++) sums[c] = total[c] % ZIGZ_BABYBEAR_P;
}

int prove(const char *path) {
    std::vector<Instance> inst;
    if (!read_instances(path, inst)) return 2;
    const size_t k = inst.size();
    // the batch through the host form's checker, values included
    std::vector<unsigned> degrees;
    std::vector<const uint64_t *> factors;
    std::vector<size_t> ns;
    for (const Instance &I : inst) {
        degrees.push_back(I.d);
        ns.push_back(I.n);
        for (unsigned j = 0; j < I.d; j++) factors.push_back(I.f[j].data());
    }
    uint64_t dummy = 0;
    size_t bad = UNTOUCHED;
    const zigz_status st = pd::check_product_batch(k, degrees.data(), (const void *const *)factors.data(), ns.data(), nullptr, &dummy,
                                                   &dummy, &dummy, &dummy, &dummy, false, true, &bad);
    if (st != ZIGZ_OK) {
        printf("check failed: status %d at %lld\n", (int)st, (long long)bad);
        return 1;
    }
    for (const Instance &I : inst) {
        {  // the host's own rounds
            Proof p;
            SumcheckRounds pr = make_prover(I, p);
            std::vector<uint64_t> f[pd::MAX_DEGREE];
            for (unsigned j = 0; j < I.d; j++) f[j] = I.f[j];
            p.fe = pr.tail_rounds(f, p.evals.data());
            if (pr.st != ZIGZ_OK) return 3;
            print_proof(p);
        }
        {  // every round from kernel-style sums
            Proof p;
            SumcheckRounds pr = make_prover(I, p);
            std::vector<uint64_t> f[pd::MAX_DEGREE];
            for (unsigned j = 0; j < I.d; j++) f[j] = I.f[j];
            for (size_t m = I.n; m > 1; m /= 2) {
                uint64_t sums[pd::MAX_DEGREE + 1], c[pd::MAX_DEGREE + 1];
                kernel_sums(I.d, f, m, sums);
                pd::coefficients(I.d, sums, c);
                const uint32_t r_m = to_mont((uint32_t)pr.step(c));
                for (unsigned j = 0; j < I.d; j++) {
                    for (size_t x = 0; x < m / 2; x++) f[j][x] = bind1((uint32_t)f[j][x], (uint32_t)f[j][x + m / 2], r_m);
                    f[j].resize(m / 2);
                }
            }
            p.fe = 1;
            for (unsigned j = 0; j < I.d; j++) {
                p.evals[j] = f[j][0];
                p.fe = f_mul(p.fe, f[j][0]);
            }
            print_proof(p);
        }
    }
    return 0;
}

// ---- the argument checks
struct Batch {  // three instances: d = 2 of 8 values, d = 3 of 4, d = 1 of 16
    std::vector<unsigned> degrees{2, 3, 1};
    std::vector<size_t> ns{8, 4, 16};
    alignas(16) uint64_t tab[6][16];
    std::vector<const void *> factors;
    std::vector<uint64_t> fixed;
    const uint64_t *fixed_p = nullptr;
    uint64_t claimed[3], rounds[64], points[16], evals[8], finals[3];
    const void *a_degrees, *a_factors, *a_ns;
    void *a_claimed, *a_rounds, *a_points, *a_evals, *a_finals;
    size_t k = 3;
    Batch() {
        for (auto &t : tab)
            for (size_t i = 0; i < 16; i++) t[i] = (1234567 * (i + 1) + (size_t)(&t - tab)) % ZIGZ_BABYBEAR_P;
        for (auto &t : tab) factors.push_back(t);
        fixed.assign(3 + 2 + 4, 5);
        for (auto *a : {claimed, finals}) std::fill(a, a + 3, SENTINEL);
        std::fill(rounds, rounds + 64, SENTINEL);
        std::fill(points, points + 16, SENTINEL);
        std::fill(evals, evals + 8, SENTINEL);
        a_degrees = degrees.data();
        a_ns = ns.data();
        a_claimed = claimed;
        a_rounds = rounds;
        a_points = points;
        a_evals = evals;
        a_finals = finals;
    }
    bool written() const {
        for (uint64_t x : claimed) if (x != SENTINEL) return true;
        for (uint64_t x : finals) if (x != SENTINEL) return true;
        for (uint64_t x : rounds) if (x != SENTINEL) return true;
        for (uint64_t x : points) if (x != SENTINEL) return true;
        for (uint64_t x : evals) if (x != SENTINEL) return true;
        return false;
    }
};

// what the entries do with a batch: every check first, then (host tables only: there is no device here) the proofs
void run_case(const char *name, Batch &b, bool dev) {
    size_t bad = UNTOUCHED;
    b.a_factors = b.factors.data();
    const unsigned *deg = (const unsigned *)b.a_degrees;
    const size_t *ns = (const size_t *)b.a_ns;
    zigz_status st;
    if (dev)
        st = pd::check_product_batch(b.k, deg, (const void *const *)b.a_factors, ns, b.fixed_p, b.a_claimed, b.a_rounds, b.a_points,
                                     b.a_evals, b.a_finals, true, false, &bad);
    else {
        st = pd::check_product_batch_host(b.k, deg, (const uint64_t *const *)b.a_factors, ns, b.fixed_p, b.a_claimed, b.a_rounds,
                                          b.a_points, b.a_evals, b.a_finals, &bad);
        // (the library finds a value >= p while it narrows the tables, before anything runs)
        if (st == ZIGZ_OK)
            st = pd::check_product_batch(b.k, deg, (const void *const *)b.a_factors, ns, b.fixed_p, b.a_claimed, b.a_rounds,
                                         b.a_points, b.a_evals, b.a_finals, false, true, &bad);
    }
    if (st == ZIGZ_OK && !dev && b.k) {
        size_t fo = 0, vo = 0, ro = 0;
        for (size_t i = 0; i < b.k; i++) {
            SumcheckRounds pr;
            pr.ncoef = deg[i] + 1;
            pr.nv = log2_floor(ns[i]);
            pr.claimed_sum = b.claimed + i;
            pr.rounds = b.rounds + ro;
            pr.point = b.points + vo;
            pr.fixed = b.fixed_p ? b.fixed_p + vo : nullptr;
            std::vector<uint64_t> f[pd::MAX_DEGREE];
            for (unsigned j = 0; j < deg[i]; j++) {
                const uint64_t *t = (const uint64_t *)b.factors[fo + j];
                f[j].assign(t, t + ns[i]);
            }
            b.finals[i] = pr.tail_rounds(f, b.evals + fo);
            fo += deg[i];
            vo += pr.nv;
            ro += pr.ncoef * pr.nv;
        }
    }
    printf("%s_%s %d %lld %d\n", name, dev ? "dev" : "host", (int)st, (long long)bad, b.written() ? 1 : 0);
}

int check() {
    for (int dev = 0; dev < 2; dev++) {
        { Batch b; run_case("ok", b, dev); }
        { Batch b; b.fixed_p = b.fixed.data(); run_case("ok_fixed", b, dev); }
        { Batch b; b.k = 0; run_case("k0", b, dev); }
        { Batch b; b.k = ZIGZ_BATCH_MAX + 1; run_case("k4097", b, dev); }
        { Batch b; b.degrees[1] = 0; run_case("degree0_1", b, dev); }
        { Batch b; b.degrees[2] = 4; run_case("degree4_2", b, dev); }
        { Batch b; b.factors[2] = nullptr; run_case("null_factor_1", b, dev); }
        { Batch b; b.factors[5] = nullptr; run_case("null_factor_2", b, dev); }
        { Batch b; b.ns[0] = 0; run_case("n0_0", b, dev); }
        { Batch b; b.ns[1] = 1; run_case("n1_1", b, dev); }
        { Batch b; b.ns[1] = 3; run_case("n3_1", b, dev); }
        { Batch b; b.ns[2] = 12; run_case("n12_2", b, dev); }
        { Batch b; b.ns[2] = (size_t)1 << 31; run_case("n2p31_2", b, dev); }
        { Batch b; b.fixed[4] = ZIGZ_BABYBEAR_P; b.fixed_p = b.fixed.data(); run_case("challenge_1", b, dev); }
        { Batch b; b.fixed[8] = ZIGZ_BABYBEAR_P - 1; b.fixed_p = b.fixed.data(); run_case("challenge_p_minus_1", b, dev); }
        { Batch b; b.a_degrees = nullptr; run_case("no_degrees", b, dev); }
        { Batch b; b.a_ns = nullptr; run_case("no_ns", b, dev); }
        { Batch b; b.a_claimed = nullptr; run_case("no_claimed", b, dev); }
        { Batch b; b.a_rounds = nullptr; run_case("no_rounds", b, dev); }
        { Batch b; b.a_points = nullptr; run_case("no_points", b, dev); }
        { Batch b; b.a_evals = nullptr; run_case("no_factor_evals", b, dev); }
        { Batch b; b.a_finals = nullptr; run_case("no_finals", b, dev); }
    }
    // device pointers: alignment (never read)
    { Batch b; b.factors[3] = (const uint8_t *)b.tab[3] + 8; run_case("misaligned_1", b, true); }
    // host tables: a value >= p, alone and in front of an instance that fails another check (the calls in order stop at it)
    { Batch b; b.tab[4][3] = ZIGZ_BABYBEAR_P; run_case("value_1", b, false); }
    { Batch b; b.tab[1][7] = ZIGZ_BABYBEAR_P; b.ns[2] = 12; run_case("value_0_before_n12_2", b, false); }
    { Batch b; b.tab[5][0] = ZIGZ_BABYBEAR_P; b.ns[1] = 3; run_case("n3_1_before_value_2", b, false); }
    { Batch b; b.tab[0][15] = ZIGZ_BABYBEAR_P; run_case("value_past_the_table", b, false); }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "prove")) return prove(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    fprintf(stderr, "usage: product_host prove FILE | check\n");
    return 2;
}
