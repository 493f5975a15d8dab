// Stand-alone driver of zigz_amd/csrc/sop_host.hpp and the rounds of sumcheck_host.hpp under it (no GPU, no HIP): built with
// -fsanitize=address,undefined by tests/test_sumcheck_sop_cpu.py and run as a child process.
//   prove FILE   FILE holds one instance per line: M n T fixed, then per term "alpha d idx_0 .. idx_{d-1}", then M * n table values,
//                then (fixed != 0) log2 n challenges.  Runs the argument checker over the whole batch (must pass), then proves
//                every instance twice and prints one line per proof -- claimed_sum final_eval, the (D + 1) v round coefficients,
//                the v challenges, the M table evaluations:
//                  first with the host's own rounds (sop::tail_rounds, what the library runs once a table is <= 1024 long),
//                  then with every round's coefficients assembled (sop::coefficients) from class sums formed the way the kernels
//                  form them: alpha into the first factor, raw 64-bit products added as low and high halves per degree class,
//                  reduced twice per 16 index pairs, i.e. carrying R^-d.
//                A third line holds the verifier's combination over the first proof (sop::verdict on pv::replay_rounds with the
//                table evaluations as oracles): its verdict as is, with final_eval + 1, and with the first table eval + 1.
//   check        runs the argument checkers on bad shapes and prints "case status bad_index written" per case (bad_index -1:
//                untouched; written: 1 if any output word changed).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "field.hpp"
#include "sop_host.hpp"

using namespace zk;

namespace {

const size_t UNTOUCHED = (size_t)-1;
const uint64_t SENTINEL = 0xA5A5A5A5A5A5A5A5ull;

struct Instance {
    unsigned M = 0, T = 0, D = 0;
    size_t n = 0;
    sop::Term terms[sop::MAX_TERMS];
    std::vector<uint64_t> f[sop::MAX_TABLES];
    std::vector<uint64_t> fixed;
};

bool read_instances(const char *path, std::vector<Instance> &out) {
    FILE *fp = fopen(path, "r");
    if (!fp) return false;
    unsigned long long M, n, T, fixed, x;
    bool ok = true;
    while (ok && fscanf(fp, "%llu %llu %llu %llu", &M, &n, &T, &fixed) == 4) {
        if (M < 1 || M > sop::MAX_TABLES || T < 1 || T > sop::MAX_TERMS || n < 2 || n > HOST_TAIL_MAX || (n & (n - 1))) { ok = false; break; }
        Instance I;
        I.M = (unsigned)M;
        I.T = (unsigned)T;
        I.n = (size_t)n;
        for (unsigned t = 0; t < I.T && ok; t++) {
            unsigned long long alpha, d;
            ok = fscanf(fp, "%llu %llu", &alpha, &d) == 2 && d >= 1 && d <= sop::MAX_DEGREE;
            I.terms[t].alpha = alpha;
            I.terms[t].d = (unsigned)d;
            for (unsigned j = 0; ok && j < d; j++) {
                ok = fscanf(fp, "%llu", &x) == 1 && x < M;
                I.terms[t].idx[j] = (uint8_t)x;
            }
            if (ok && d > I.D) I.D = (unsigned)d;
        }
        for (unsigned j = 0; j < I.M && ok; j++)
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
    p.rounds.assign((I.D + 1) * v, SENTINEL);
    p.point.assign(v, SENTINEL);
    p.evals.assign(I.M, SENTINEL);
    SumcheckRounds pr;
    pr.ncoef = I.D + 1;
    pr.nv = v;
    pr.claimed_sum = &p.claimed;
    pr.rounds = p.rounds.data();
    pr.point = p.point.data();
    pr.fixed = I.fixed.empty() ? nullptr : I.fixed.data();
    return pr;
}

// the SUMS class sums of one round as sumcheck_sop.hip forms them (sop_terms1 / pd_terms / sop_store): per group of 16 index
// pairs and degree class the raw 64-bit products of all terms added as low and high halves and reduced twice (class 1: the plain
// sum), the groups' values added and reduced mod p once
void kernel_sums(const Instance &I, const std::vector<uint64_t> *f, size_t m, uint64_t *sums) {
    const size_t half = m / 2;
    uint64_t total[sop::SUMS] = {};
    for (size_t g0 = 0; g0 < half; g0 += 16) {
        uint64_t lo[sop::SUMS] = {}, hi[sop::SUMS] = {};
        auto add = [&](unsigned c, uint32_t x, uint32_t y) {
            const uint64_t pr = (uint64_t)x * y;
            lo[c] += (uint32_t)pr;
            hi[c] += pr >> 32;
        };
        for (size_t i = g0; i < g0 + 16 && i < half; i++)
            for (unsigned t = 0; t < I.T; t++) {
                const sop::Term &tm = I.terms[t];
                const uint32_t alpha_m = to_mont((uint32_t)tm.alpha);
                uint32_t a[sop::MAX_DEGREE], e[sop::MAX_DEGREE];
                for (unsigned j = 0; j < tm.d; j++) {
                    uint32_t lo_v = (uint32_t)f[tm.idx[j]][i], hi_v = (uint32_t)f[tm.idx[j]][i + half];
                    if (j == 0) {
                        lo_v = mont_mul(alpha_m, lo_v);
                        hi_v = mont_mul(alpha_m, hi_v);
                    }
                    a[j] = lo_v;
                    e[j] = sub_mod(hi_v, lo_v);
                }
                const unsigned at = sop::CLASS_AT[tm.d - 1];
                if (tm.d == 1) {
                    lo[at] += a[0];
                    lo[at + 1] += e[0];
                } else if (tm.d == 2) {
                    add(at, a[0], a[1]);
                    add(at + 1, a[0], e[1]);
                    add(at + 1, e[0], a[1]);
                    add(at + 2, e[0], e[1]);
                } else {
                    const uint32_t p = mont_mul(a[0], a[1]), q = mont_mul(e[0], e[1]);
                    const uint32_t x = monty_reduce((uint64_t)a[0] * e[1] + (uint64_t)e[0] * a[1]);
                    add(at, p, a[2]);
                    add(at + 1, p, e[2]);
                    add(at + 1, x, a[2]);
                    add(at + 2, x, e[2]);
                    add(at + 2, q, a[2]);
                    add(at + 3, q, e[2]);
                }
            }
        for (unsigned c = 0; c < sop::SUMS; c++) total[c] += c < sop::CLASS_AT[1] ? lo[c] : (uint64_t)monty_reduce(hi[c] + monty_reduce(lo[c]));
    }
    for (unsigned c = 0; c < sop::SUMS; c++) sums[c] = total[c] % ZIGZ_BABYBEAR_P;
}

int prove(const char *path) {
    std::vector<Instance> inst;
    if (!read_instances(path, inst)) return 2;
    // the batch through the host form's checker, values included
    std::vector<unsigned> n_tables, n_terms, degrees;
    std::vector<uint8_t> idx;
    std::vector<uint64_t> coeffs;
    std::vector<const void *> tables;
    std::vector<size_t> ns;
    for (const Instance &I : inst) {
        n_tables.push_back(I.M);
        n_terms.push_back(I.T);
        ns.push_back(I.n);
        for (unsigned j = 0; j < I.M; j++) tables.push_back(I.f[j].data());
        for (unsigned t = 0; t < I.T; t++) {
            degrees.push_back(I.terms[t].d);
            coeffs.push_back(I.terms[t].alpha);
            idx.insert(idx.end(), I.terms[t].idx, I.terms[t].idx + I.terms[t].d);
        }
    }
    uint64_t dummy = 0;
    size_t bad = UNTOUCHED;
    const sop::Args a{inst.size(), n_tables.data(), tables.data(), ns.data(), n_terms.data(), degrees.data(), idx.data(), coeffs.data(),
                      nullptr, &dummy, &dummy, &dummy, &dummy, &dummy};
    const zigz_status st = sop::check_sop_batch(a, false, true, &bad);
    if (st != ZIGZ_OK) {
        printf("check failed: status %d at %lld\n", (int)st, (long long)bad);
        return 1;
    }
    // (the library's view of the flat arrays gives the driver's terms back)
    const std::vector<sop::Shape> sh = sop::shapes(inst.size(), n_tables.data(), ns.data(), n_terms.data(), degrees.data(), idx.data(), coeffs.data());
    for (size_t x = 0; x < inst.size(); x++) {
        const Instance &I = inst[x];
        if (sh[x].M != I.M || sh[x].T != I.T || sh[x].D != I.D) return 4;
        Proof first;
        {  // the host's own rounds
            SumcheckRounds pr = make_prover(I, first);
            std::vector<uint64_t> f[sop::MAX_TABLES];
            for (unsigned j = 0; j < I.M; j++) f[j] = I.f[j];
            first.fe = sop::tail_rounds(pr, f, I.M, sh[x].terms, I.T, first.evals.data());
            if (pr.st != ZIGZ_OK) return 3;
            print_proof(first);
        }
        {  // every round from kernel-style class sums
            Proof p;
            SumcheckRounds pr = make_prover(I, p);
            std::vector<uint64_t> f[sop::MAX_TABLES];
            for (unsigned j = 0; j < I.M; j++) f[j] = I.f[j];
            for (size_t m = I.n; m > 1; m /= 2) {
                uint64_t sums[sop::SUMS], c[sop::MAX_DEGREE + 1];
                kernel_sums(I, f, m, sums);
                sop::coefficients(I.D, sums, c);
                const uint32_t r_m = to_mont((uint32_t)pr.step(c));
                for (unsigned j = 0; j < I.M; j++) {
                    for (size_t i = 0; i < m / 2; i++) f[j][i] = bind1((uint32_t)f[j][i], (uint32_t)f[j][i + m / 2], r_m);
                    f[j].resize(m / 2);
                }
            }
            for (unsigned j = 0; j < I.M; j++) p.evals[j] = f[j][0];
            p.fe = sop::combine(I.terms, I.T, p.evals.data());
            print_proof(p);
        }
        {  // the verifier's combination
            const sv::Replay rep = pv::replay_rounds(first.claimed, first.rounds.data(), first.point.size(), I.D);
            std::vector<uint64_t> wrong = first.evals;
            wrong[0] = f_add(wrong[0], 1);
            printf("%d %d %d\n", (int)sop::verdict(rep, I.terms, I.T, first.evals.data(), I.M, first.fe, first.evals.data()),
                   (int)sop::verdict(rep, I.terms, I.T, first.evals.data(), I.M, f_add(first.fe, 1), first.evals.data()),
                   (int)sop::verdict(rep, I.terms, I.T, first.evals.data(), I.M, first.fe, wrong.data()));
        }
    }
    return 0;
}

// ---- the argument checks
struct Batch {  // three instances: pool of 2 (8 values), terms (a; 0 1), (b; 1) | pool of 3 (4), term (c; 0 1 2) | pool of 1 (16), term (d; 0)
    std::vector<unsigned> n_tables{2, 3, 1}, n_terms{2, 1, 1}, degrees{2, 1, 3, 1};
    std::vector<uint8_t> idx{0, 1, 1, 0, 1, 2, 0};
    std::vector<uint64_t> coeffs{7, 0, ZIGZ_BABYBEAR_P - 1, 1};
    std::vector<size_t> ns{8, 4, 16};
    alignas(16) uint64_t tab[6][16];
    std::vector<const void *> tables;
    std::vector<uint64_t> fixed;
    const uint64_t *fixed_p = nullptr;
    uint64_t claimed[3], rounds[64], points[16], evals[8], finals[3];
    const void *a_n_tables, *a_ns, *a_n_terms, *a_degrees, *a_idx, *a_coeffs;
    void *a_claimed, *a_rounds, *a_points, *a_evals, *a_finals;
    size_t k = 3;
    Batch() {
        for (auto &t : tab)
            for (size_t i = 0; i < 16; i++) t[i] = (1234567 * (i + 1) + (size_t)(&t - tab)) % ZIGZ_BABYBEAR_P;
        for (auto &t : tab) tables.push_back(t);
        fixed.assign(3 + 2 + 4, 5);
        for (auto *a : {claimed, finals}) std::fill(a, a + 3, SENTINEL);
        std::fill(rounds, rounds + 64, SENTINEL);
        std::fill(points, points + 16, SENTINEL);
        std::fill(evals, evals + 8, SENTINEL);
        a_n_tables = n_tables.data();
        a_ns = ns.data();
        a_n_terms = n_terms.data();
        a_degrees = degrees.data();
        a_idx = idx.data();
        a_coeffs = coeffs.data();
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
    const sop::Args a{b.k, (const unsigned *)b.a_n_tables, b.tables.data(), (const size_t *)b.a_ns, (const unsigned *)b.a_n_terms,
                      (const unsigned *)b.a_degrees, (const uint8_t *)b.a_idx, (const uint64_t *)b.a_coeffs, b.fixed_p,
                      b.a_claimed, b.a_rounds, b.a_points, b.a_evals, b.a_finals};
    zigz_status st;
    if (dev)
        st = sop::check_sop_batch(a, true, false, &bad);
    else {
        st = sop::check_sop_batch_host(a, &bad);
        // (the library finds a value >= p while it narrows the tables, before anything runs)
        if (st == ZIGZ_OK) st = sop::check_sop_batch(a, false, true, &bad);
    }
    if (st == ZIGZ_OK && !dev && b.k) {
        const std::vector<sop::Shape> sh = sop::shapes(a.k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs);
        for (size_t i = 0; i < b.k; i++) {
            SumcheckRounds pr;
            pr.ncoef = sh[i].D + 1;
            pr.nv = sh[i].nv;
            pr.claimed_sum = b.claimed + i;
            pr.rounds = b.rounds + sh[i].roff;
            pr.point = b.points + sh[i].voff;
            pr.fixed = b.fixed_p ? b.fixed_p + sh[i].voff : nullptr;
            std::vector<uint64_t> f[sop::MAX_TABLES];
            for (unsigned j = 0; j < sh[i].M; j++) {
                const uint64_t *t = (const uint64_t *)b.tables[sh[i].moff + j];
                f[j].assign(t, t + a.ns[i]);
            }
            b.finals[i] = sop::tail_rounds(pr, f, sh[i].M, sh[i].terms, sh[i].T, b.evals + sh[i].moff);
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
        { Batch b; b.n_tables[1] = 0; run_case("pool0_1", b, dev); }
        { Batch b; b.n_tables[2] = 9; run_case("pool9_2", b, dev); }
        { Batch b; b.n_terms[0] = 0; run_case("terms0_0", b, dev); }
        { Batch b; b.n_terms[1] = 9; run_case("terms9_1", b, dev); }
        { Batch b; b.degrees[1] = 0; run_case("degree0_0", b, dev); }
        { Batch b; b.degrees[3] = 4; run_case("degree4_2", b, dev); }
        { Batch b; b.idx[1] = 2; run_case("index2_0", b, dev); }
        { Batch b; b.idx[5] = 3; run_case("index3_1", b, dev); }
        { Batch b; b.tables[2] = nullptr; run_case("null_table_1", b, dev); }
        { Batch b; b.tables[5] = nullptr; run_case("null_table_2", b, dev); }
        { Batch b; b.ns[0] = 0; run_case("n0_0", b, dev); }
        { Batch b; b.ns[1] = 1; run_case("n1_1", b, dev); }
        { Batch b; b.ns[1] = 3; run_case("n3_1", b, dev); }
        { Batch b; b.ns[2] = 12; run_case("n12_2", b, dev); }
        { Batch b; b.ns[2] = (size_t)1 << 31; run_case("n2p31_2", b, dev); }
        { Batch b; b.fixed[4] = ZIGZ_BABYBEAR_P; b.fixed_p = b.fixed.data(); run_case("challenge_1", b, dev); }
        { Batch b; b.fixed[8] = ZIGZ_BABYBEAR_P - 1; b.fixed_p = b.fixed.data(); run_case("challenge_p_minus_1", b, dev); }
        { Batch b; b.coeffs[2] = ZIGZ_BABYBEAR_P; run_case("coeff_1", b, dev); }
        // the family's order within one instance: the terms before the shape, the shape before the coefficient
        { Batch b; b.idx[5] = 3; b.ns[1] = 3; run_case("index3_1_before_n3_1", b, dev); }
        { Batch b; b.ns[1] = 3; b.coeffs[2] = ZIGZ_BABYBEAR_P; run_case("n3_1_before_coeff_1", b, dev); }
        // ... and the first failing instance wins
        { Batch b; b.coeffs[0] = ZIGZ_BABYBEAR_P; b.n_tables[1] = 0; run_case("coeff_0_before_pool0_1", b, dev); }
        { Batch b; b.a_n_tables = nullptr; run_case("no_n_tables", b, dev); }
        { Batch b; b.a_ns = nullptr; run_case("no_ns", b, dev); }
        { Batch b; b.a_n_terms = nullptr; run_case("no_n_terms", b, dev); }
        { Batch b; b.a_degrees = nullptr; run_case("no_degrees", b, dev); }
        { Batch b; b.a_idx = nullptr; run_case("no_term_tables", b, dev); }
        { Batch b; b.a_coeffs = nullptr; run_case("no_coeffs", b, dev); }
        { Batch b; b.a_claimed = nullptr; run_case("no_claimed", b, dev); }
        { Batch b; b.a_rounds = nullptr; run_case("no_rounds", b, dev); }
        { Batch b; b.a_points = nullptr; run_case("no_points", b, dev); }
        { Batch b; b.a_evals = nullptr; run_case("no_table_evals", b, dev); }
        { Batch b; b.a_finals = nullptr; run_case("no_finals", b, dev); }
    }
    // device pointers: alignment (never read)
    { Batch b; b.tables[3] = (const uint8_t *)b.tab[3] + 8; run_case("misaligned_1", b, true); }
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
    fprintf(stderr, "usage: sop_host prove FILE | check\n");
    return 2;
}
