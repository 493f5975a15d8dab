// Stand-alone driver of zigz_amd/csrc/zerocheck_host.hpp (no GPU, no HIP): built with -fsanitize=address,undefined by
// tests/test_zerocheck_closed_cpu.py and run as a child process.
//   prove FILE L   FILE holds one instance per line: M n T fixed, then per term "alpha d idx_0 .. idx_{d-1}", then log2 n words of tau,
//                  then M * n table values, then (fixed != 0) log2 n challenges.  Runs the argument checker over the whole batch (must
//                  pass), then proves every instance twice and prints one line per proof -- claimed_sum final_eval eq_eval, the
//                  (D + 2) v round coefficients, the v challenges, the M table evaluations:
//                    first with the host's own rounds from the full tables (zc::tail_rounds);
//                    then with every round of 2^L pairs or more assembled (sop::coefficients, zc::Weight::step) from class sums formed
//                    the way the kernels form them -- the pair's weight lo[x & (2^L - 1)] * hi_r[x >> L] from zc::build_weights, in
//                    Montgomery form, multiplied into alpha and then into the term's first factor, raw 64-bit products added as low and
//                    high halves per degree class and reduced twice per block of 2^L pairs, the blocks' values added and reduced once --
//                    and the shorter rounds by zc::tail_rounds, as the library hands over.
//                  A third line holds zc::verdict over the first proof with its own evaluations as oracles: as is, with final_eval + 1,
//                  with eq_eval + 1.
//   check          checks the stage every pass of a live instance reads (zc::stage, zc::weight_words) against the stages there are, at
//                  every v from 11 to ZIGZ_PRODUCT_MAX_LOG2_N (exit status 6); then runs the argument checkers on bad shapes and
//                  prints "case status bad_index" per case (bad_index -1: untouched).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "field.hpp"
#include "zerocheck_host.hpp"

using namespace zk;

namespace {

const size_t UNTOUCHED = (size_t)-1;
const uint64_t SENTINEL = 0xA5A5A5A5A5A5A5A5ull;

struct Instance {
    unsigned M = 0, T = 0, D = 0;
    size_t n = 0;
    sop::Term terms[sop::MAX_TERMS];
    std::vector<uint64_t> tau;
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
        for (size_t r = 0; ok && r < log2_floor(I.n); r++) {
            ok = fscanf(fp, "%llu", &x) == 1;
            I.tau.push_back(x);
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
    uint64_t claimed = SENTINEL, fe = SENTINEL, eq = SENTINEL;
    std::vector<uint64_t> rounds, point, evals;
};

void print_proof(const Proof &p) {
    printf("%llu %llu %llu", (unsigned long long)p.claimed, (unsigned long long)p.fe, (unsigned long long)p.eq);
    for (uint64_t x : p.rounds) printf(" %llu", (unsigned long long)x);
    for (uint64_t x : p.point) printf(" %llu", (unsigned long long)x);
    for (uint64_t x : p.evals) printf(" %llu", (unsigned long long)x);
    printf("\n");
}

SumcheckRounds make_prover(const Instance &I, Proof &p) {
    const size_t v = log2_floor(I.n);
    p.rounds.assign((I.D + 2) * v, SENTINEL);
    p.point.assign(v, SENTINEL);
    p.evals.assign(I.M, SENTINEL);
    SumcheckRounds pr;
    pr.ncoef = I.D + 2;
    pr.nv = v;
    pr.claimed_sum = &p.claimed;
    pr.rounds = p.rounds.data();
    pr.point = p.point.data();
    pr.fixed = I.fixed.empty() ? nullptr : I.fixed.data();
    return pr;
}

void finish(const Instance &I, Proof &p, uint64_t c) {
    p.eq = pv::eq_at(I.tau.data(), p.point.data(), p.point.size(), true);
    p.fe = f_mul(p.eq, c);
}

// the SUMS class sums of one round of m / 2 >= 2^L pairs as sumcheck_zerocheck.hip forms them: per block of 2^L pairs (one trip
// of a workgroup: hi uniform, lo indexed by the pair's low bits) and degree class the raw 64-bit products of all terms added as low
// and high halves and reduced twice (class 1: the plain sum), the blocks' values added and reduced mod p once
void kernel_sums(const Instance &I, const std::vector<uint64_t> *f, size_t m, unsigned L, const uint32_t *lo_m, const uint32_t *hi_m,
                 uint64_t *sums) {
    const size_t half = m / 2, block = (size_t)1 << L;
    const uint32_t *stage = hi_m + zc::stage_at(log2_floor(half) - L);
    uint64_t total[sop::SUMS] = {};
    for (size_t g = 0; g < half / block; g++) {
        uint64_t lo[sop::SUMS] = {}, hi[sop::SUMS] = {};
        auto add = [&](unsigned c, uint32_t x, uint32_t y) {
            const uint64_t pr = (uint64_t)x * y;
            lo[c] += (uint32_t)pr;
            hi[c] += pr >> 32;
        };
        const uint32_t h_m = stage[g];
        for (size_t i = g * block; i < (g + 1) * block; i++) {
            const uint32_t w_m = mont_mul(lo_m[i & (block - 1)], h_m);
            for (unsigned t = 0; t < I.T; t++) {
                const sop::Term &tm = I.terms[t];
                const uint32_t cw = mont_mul(to_mont((uint32_t)tm.alpha), w_m);
                uint32_t a[sop::MAX_DEGREE], e[sop::MAX_DEGREE];
                for (unsigned j = 0; j < tm.d; j++) {
                    uint32_t lo_v = (uint32_t)f[tm.idx[j]][i], hi_v = (uint32_t)f[tm.idx[j]][i + half];
                    if (j == 0) {
                        lo_v = mont_mul(cw, lo_v);
                        hi_v = mont_mul(cw, hi_v);
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
        }
        for (unsigned c = 0; c < sop::SUMS; c++) total[c] += c < sop::CLASS_AT[1] ? lo[c] : (uint64_t)monty_reduce(hi[c] + monty_reduce(lo[c]));
    }
    for (unsigned c = 0; c < sop::SUMS; c++) sums[c] = total[c] % ZIGZ_BABYBEAR_P;
}

struct Flat {  // the entries' flat arrays of a list of instances
    std::vector<unsigned> n_tables, n_terms, degrees;
    std::vector<uint8_t> idx;
    std::vector<uint64_t> coeffs, taus;
    std::vector<const void *> tables;
    std::vector<size_t> ns;
    explicit Flat(const std::vector<Instance> &inst) {
        for (const Instance &I : inst) {
            n_tables.push_back(I.M);
            n_terms.push_back(I.T);
            ns.push_back(I.n);
            taus.insert(taus.end(), I.tau.begin(), I.tau.end());
            for (unsigned j = 0; j < I.M; j++) tables.push_back(I.f[j].data());
            for (unsigned t = 0; t < I.T; t++) {
                degrees.push_back(I.terms[t].d);
                coeffs.push_back(I.terms[t].alpha);
                idx.insert(idx.end(), I.terms[t].idx, I.terms[t].idx + I.terms[t].d);
            }
        }
    }
};

int prove(const char *path, unsigned L) {
    std::vector<Instance> inst;
    if (!read_instances(path, inst)) return 2;
    const Flat fl(inst);
    uint64_t dummy = 0;
    size_t bad = UNTOUCHED;
    const zc::Args a{{inst.size(), fl.n_tables.data(), fl.tables.data(), fl.ns.data(), fl.n_terms.data(), fl.degrees.data(), fl.idx.data(),
                      fl.coeffs.data(), nullptr, &dummy, &dummy, &dummy, &dummy, &dummy},
                     fl.taus.data(), &dummy};
    const zigz_status st = zc::check_zerocheck_batch(a, false, true, &bad);
    if (st != ZIGZ_OK) {
        printf("check failed: status %d at %lld\n", (int)st, (long long)bad);
        return 1;
    }
    const std::vector<sop::Shape> sh =
        sop::shapes(inst.size(), fl.n_tables.data(), fl.ns.data(), fl.n_terms.data(), fl.degrees.data(), fl.idx.data(), fl.coeffs.data());
    const std::vector<size_t> roff = zc::round_offsets(sh);
    for (size_t x = 0; x < inst.size(); x++) {
        const Instance &I = inst[x];
        const unsigned v = log2_floor(I.n);
        if (sh[x].M != I.M || sh[x].T != I.T || sh[x].D != I.D || roff[x + 1] - roff[x] != (size_t)(I.D + 2) * v) return 4;
        Proof first;
        {  // the host's own rounds
            SumcheckRounds pr = make_prover(I, first);
            zc::Weight w{I.tau.data(), v, 1};
            std::vector<uint64_t> f[sop::MAX_TABLES];
            for (unsigned j = 0; j < I.M; j++) f[j] = I.f[j];
            const uint64_t c = zc::tail_rounds(pr, w, f, I.M, sh[x].terms, I.T, I.D, first.evals.data());
            if (pr.st != ZIGZ_OK) return 3;
            finish(I, first, c);
            if (w.P != first.eq) return 5;  // the prefix scalar after the last round IS eq at the reversed point
            print_proof(first);
        }
        {  // the long rounds from kernel-style weighted class sums, the rest by the host's rounds
            Proof p;
            SumcheckRounds pr = make_prover(I, p);
            zc::Weight w{I.tau.data(), v, 1};
            std::vector<uint64_t> f[sop::MAX_TABLES];
            for (unsigned j = 0; j < I.M; j++) f[j] = I.f[j];
            std::vector<uint32_t> lo_m, hi_m;
            if (v > L) {
                lo_m.assign((size_t)1 << L, 0xFFFFFFFFu);
                hi_m.assign(zc::hi_words(v, L), 0xFFFFFFFFu);
                zc::build_weights(I.tau.data(), v, L, lo_m.data(), hi_m.data());
            }
            size_t m = I.n;
            for (; m / 2 >= ((size_t)1 << L) && m > 1; m /= 2) {
                uint64_t sums[sop::SUMS], c[sop::MAX_DEGREE + 1];
                kernel_sums(I, f, m, L, lo_m.data(), hi_m.data(), sums);
                sop::coefficients(I.D, sums, c);
                const uint32_t r_m = to_mont((uint32_t)w.step(pr, I.D, c));
                if (pr.st != ZIGZ_OK) return 3;
                for (unsigned j = 0; j < I.M; j++) {
                    for (size_t i = 0; i < m / 2; i++) f[j][i] = bind1((uint32_t)f[j][i], (uint32_t)f[j][i + m / 2], r_m);
                    f[j].resize(m / 2);
                }
            }
            const uint64_t c = zc::tail_rounds(pr, w, f, I.M, sh[x].terms, I.T, I.D, p.evals.data());
            if (pr.st != ZIGZ_OK) return 3;
            finish(I, p, c);
            print_proof(p);
        }
        {  // the verifier's verdict, at D + 2 coefficients per round
            const sv::Replay rep = pv::replay_rounds(first.claimed, first.rounds.data(), first.point.size(), I.D + 1);
            const uint64_t wrong = f_add(first.eq, 1);
            printf("%d %d %d\n",
                   (int)zc::verdict(rep, I.terms, I.T, first.evals.data(), I.M, first.eq, first.fe, first.evals.data(), &first.eq),
                   (int)zc::verdict(rep, I.terms, I.T, first.evals.data(), I.M, first.eq, f_add(first.fe, 1), first.evals.data(), &first.eq),
                   (int)zc::verdict(rep, I.terms, I.T, first.evals.data(), I.M, first.eq, first.fe, first.evals.data(), &wrong));
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
    std::vector<uint64_t> taus{3, 0, ZIGZ_BABYBEAR_P - 1, 1, 9, 2, 4, 6, 8};  // 3 + 2 + 4 words
    alignas(16) uint64_t tab[6][16];
    std::vector<const void *> tables;
    std::vector<uint64_t> fixed;
    const uint64_t *fixed_p = nullptr;
    // the proof words of the verifier's cases: canonical zeros, (D + 2) v = 4*3 + 5*2 + 3*4 round words
    uint64_t claimed[3] = {}, rounds[64] = {}, points[16] = {}, evals[8] = {}, eqs[3] = {}, finals[3] = {};
    const void *a_n_tables, *a_ns, *a_n_terms, *a_degrees, *a_idx, *a_coeffs, *a_taus;
    void *a_claimed, *a_rounds, *a_points, *a_evals, *a_eqs, *a_finals;
    size_t k = 3;
    Batch() {
        for (auto &t : tab)
            for (size_t i = 0; i < 16; i++) t[i] = (1234567 * (i + 1) + (size_t)(&t - tab)) % ZIGZ_BABYBEAR_P;
        for (auto &t : tab) tables.push_back(t);
        fixed.assign(3 + 2 + 4, 5);
        a_n_tables = n_tables.data();
        a_ns = ns.data();
        a_n_terms = n_terms.data();
        a_degrees = degrees.data();
        a_idx = idx.data();
        a_coeffs = coeffs.data();
        a_taus = taus.data();
        a_claimed = claimed;
        a_rounds = rounds;
        a_points = points;
        a_evals = evals;
        a_eqs = eqs;
        a_finals = finals;
    }
};

void run_case(const char *name, Batch &b, bool dev) {
    size_t bad = UNTOUCHED;
    const zc::Args a{{b.k, (const unsigned *)b.a_n_tables, b.tables.data(), (const size_t *)b.a_ns, (const unsigned *)b.a_n_terms,
                      (const unsigned *)b.a_degrees, (const uint8_t *)b.a_idx, (const uint64_t *)b.a_coeffs, b.fixed_p, b.a_claimed,
                      b.a_rounds, b.a_points, b.a_evals, b.a_finals},
                     (const uint64_t *)b.a_taus, b.a_eqs};
    zigz_status st;
    if (dev)
        st = zc::check_zerocheck_batch(a, true, false, &bad);
    else {
        st = zc::check_zerocheck_batch_host(a, &bad);
        // (the library finds a value >= p while it narrows the tables, before anything runs)
        if (st == ZIGZ_OK) st = zc::check_zerocheck_batch(a, false, true, &bad);
    }
    printf("%s_%s %d %lld\n", name, dev ? "dev" : "host", (int)st, (long long)bad);
}

void run_verify_case(const char *name, Batch &b, uint32_t flags, bool no_rejected = false) {
    size_t bad = UNTOUCHED, rejected = 0;
    const zc::VerifyArgs a{b.k, (const unsigned *)b.a_n_tables, b.tables.data(), (const uint64_t *)b.a_taus, (const size_t *)b.a_ns,
                           (const unsigned *)b.a_n_terms, (const unsigned *)b.a_degrees, (const uint8_t *)b.a_idx,
                           (const uint64_t *)b.a_coeffs, (const uint64_t *)b.a_claimed, (const uint64_t *)b.a_rounds,
                           (const uint64_t *)b.a_points, (const uint64_t *)b.a_evals, (const uint64_t *)b.a_eqs,
                           (const uint64_t *)b.a_finals, flags, no_rejected ? nullptr : &rejected};
    for (int dev = 0; dev < 2; dev++) {
        bad = UNTOUCHED;
        const zigz_status st = dev ? zc::check_verify_zerocheck_batch(a, true, false, &bad) : zc::check_verify_zerocheck_batch_host(a, &bad);
        printf("verify_%s_%s %d %lld\n", name, dev ? "dev" : "host", (int)st, (long long)bad);
    }
}

// The stage a pass reads, at every live length of an instance of 2^v values (round 0 at 2^v, then one bind pass per length down
// to 2048): the stage's first word and the pairs / 1024 words (at least one) the pass reads from it lie inside the hi stages
// build_weights wrote and inside the instance's share of the weights region, whose size keeps the next instance's lo 16-byte aligned
bool stages_in_bounds() {
    const size_t lo = (size_t)1 << zc::LOG2_LO;
    for (unsigned v = zc::LOG2_LO + 1; v <= ZIGZ_PRODUCT_MAX_LOG2_N; v++) {
        const size_t n = (size_t)1 << v, words = zc::weight_words(n), hi = zc::hi_words(v, zc::LOG2_LO);
        if (words % 4 || lo + hi > words) {
            fprintf(stderr, "weight_words(2^%u) = %zu: not a multiple of 4 words, or short of lo + %zu\n", v, words, hi);
            return false;
        }
        for (int bind = 0; bind < 2; bind++)
            for (size_t m = n; m > HOST_TAIL_MAX; m = bind ? m / 2 : HOST_TAIL_MAX) {
                const size_t reads = std::max(zc::pairs(m, bind) / lo, (size_t)1), end = zc::stage_at(zc::stage(m, bind)) + reads;
                if (end > hi || lo + end > words) {
                    fprintf(stderr, "v %u, %s pass at m = %zu: stage %u, words [%zu, %zu) of %zu hi words\n", v, bind ? "bind" : "sums", m,
                            zc::stage(m, bind), zc::stage_at(zc::stage(m, bind)), end, hi);
                    return false;
                }
            }
    }
    return true;
}

int check() {
    if (!stages_in_bounds()) return 6;
    const uint64_t p = ZIGZ_BABYBEAR_P;
    for (int dev = 0; dev < 2; dev++) {
        { Batch b; run_case("ok", b, dev); }
        { Batch b; b.fixed_p = b.fixed.data(); run_case("ok_fixed", b, dev); }
        { Batch b; b.k = 0; run_case("k0", b, dev); }
        { Batch b; b.k = 0; b.a_taus = nullptr; run_case("k0_no_eq_points", b, dev); }
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
        { Batch b; b.ns[0] = 0; run_case("n0_0", b, dev); }
        { Batch b; b.ns[1] = 1; run_case("n1_1", b, dev); }
        { Batch b; b.ns[1] = 3; run_case("n3_1", b, dev); }
        { Batch b; b.ns[2] = 12; run_case("n12_2", b, dev); }
        { Batch b; b.ns[2] = (size_t)1 << 31; run_case("n2p31_2", b, dev); }
        { Batch b; b.fixed[4] = p; b.fixed_p = b.fixed.data(); run_case("challenge_1", b, dev); }
        { Batch b; b.coeffs[2] = p; run_case("coeff_1", b, dev); }
        // tau: a word >= p, in every instance's place; p - 1, 0 and 1 are values like any other (the ok batch holds them)
        { Batch b; b.taus[0] = p; run_case("tau_0", b, dev); }
        { Batch b; b.taus[4] = p; run_case("tau_1", b, dev); }
        { Batch b; b.taus[8] = ~(uint64_t)0; run_case("tau_2", b, dev); }
        // the order: within an instance the shape comes before tau; the first failing instance wins, whichever check it fails
        { Batch b; b.taus[3] = p; b.ns[1] = 3; run_case("n3_1_before_tau_1", b, dev); }
        { Batch b; b.taus[0] = p; b.ns[1] = 3; run_case("tau_0_before_n3_1", b, dev); }
        { Batch b; b.taus[5] = p; b.ns[1] = 3; run_case("n3_1_before_tau_2", b, dev); }
        { Batch b; b.taus[0] = p; b.coeffs[2] = p; run_case("tau_0_before_coeff_1", b, dev); }
        { Batch b; b.a_n_tables = nullptr; run_case("no_n_tables", b, dev); }
        { Batch b; b.a_ns = nullptr; run_case("no_ns", b, dev); }
        { Batch b; b.a_coeffs = nullptr; run_case("no_coeffs", b, dev); }
        { Batch b; b.a_taus = nullptr; run_case("no_eq_points", b, dev); }
        { Batch b; b.a_eqs = nullptr; run_case("no_eq_evals", b, dev); }
        { Batch b; b.a_evals = nullptr; run_case("no_table_evals", b, dev); }
        { Batch b; b.a_finals = nullptr; run_case("no_finals", b, dev); }
    }
    { Batch b; b.tables[3] = (const uint8_t *)b.tab[3] + 8; run_case("misaligned_1", b, true); }
    // host tables: a value >= p in front of the instance whose tau fails is reported instead; behind it, it is not
    { Batch b; b.tab[4][3] = p; run_case("value_1", b, false); }
    { Batch b; b.tab[1][7] = p; b.taus[4] = p; run_case("value_0_before_tau_1", b, false); }
    { Batch b; b.tab[5][0] = p; b.taus[4] = p; run_case("tau_1_before_value_2", b, false); }
    // the verifier's checker
    { Batch b; run_verify_case("ok", b, ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED); }
    { Batch b; run_verify_case("ok_flags0", b, 0); }
    { Batch b; run_verify_case("flags2", b, 2); }
    { Batch b; run_verify_case("no_n_rejected", b, 0, true); }
    { Batch b; b.k = 0; b.a_taus = nullptr; run_verify_case("k0", b, 0); }
    { Batch b; b.a_taus = nullptr; run_verify_case("no_eq_points", b, 0); }
    { Batch b; b.a_evals = nullptr; b.a_eqs = nullptr; run_verify_case("no_evals_is_ok", b, 0); }
    { Batch b; b.a_finals = nullptr; run_verify_case("no_finals", b, 0); }
    { Batch b; b.degrees[3] = 4; run_verify_case("degree4_2", b, 0); }
    { Batch b; b.ns[1] = 1; run_verify_case("n1_1", b, 0); }
    { Batch b; b.taus[4] = p; run_verify_case("tau_1", b, 0); }
    { Batch b; b.eqs[2] = p; run_verify_case("eq_eval_2", b, 0); }
    { Batch b; b.rounds[11] = p; run_verify_case("round_word_0_last", b, 0); }       // instance 0: 4 x 3 words
    { Batch b; b.rounds[12 + 9] = p; run_verify_case("round_word_1_last", b, 0); }   // instance 1: 5 x 2 words (degree 3 + eq)
    { Batch b; b.rounds[22 + 11] = p; run_verify_case("round_word_2_last", b, 0); }  // instance 2: 3 x 4 words
    { Batch b; b.rounds[34] = p; run_verify_case("word_behind_the_rounds", b, 0); }
    { Batch b; b.points[3] = p; run_verify_case("point_1", b, 0); }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "prove")) return prove(argv[2], (unsigned)atoi(argv[3]));
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    fprintf(stderr, "usage: zerocheck_host prove FILE L | check\n");
    return 2;
}
