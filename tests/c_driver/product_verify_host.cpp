// Stand-alone driver of zigz_amd/csrc/product_verify_host.hpp (no GPU, no HIP): built with -fsanitize=address,undefined by
// tests/test_zerocheck_cpu.py and run as a child process.
//   verify FILE   FILE holds one proof per line: d v reversed check_factor_evals claimed_sum final_eval, then (d + 1) v round
//                 coefficients, v point coordinates, d factor evals, and per factor either "0 value" (a table: its extension at the
//                 evaluation point, computed by the caller) or "1 tau_0 .. tau_{v-1}" (eq(tau, .)).  Runs the device form's argument
//                 checker over every proof (must pass), then prints per proof "verdict rounds_ok expected_eval oracle_0 .. " and,
//                 for d = 1, a last word: 1 if pv::replay_rounds equals sv::replay_rounds.
//   time FILE R   the replays (and eq factors) of FILE's proofs on the library's host threads, R times after a warm-up: prints
//                 "replay_ms median min max rounds_ok" (tools/eq_table_rate.py: the host's share alone)
//   check         runs the argument checkers on bad shapes and prints "case status bad_index" per case (bad_index -1: untouched).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "host_parallel.hpp"
#include "product_verify_host.hpp"

using namespace zk;

namespace {

const size_t UNTOUCHED = (size_t)-1;

struct Proof {
    unsigned d = 0;
    size_t v = 0;
    bool reversed = false, check_fe = false;
    uint64_t claimed = 0, final_eval = 0;
    std::vector<uint64_t> rounds, point, fevals, table_evals, taus;
    std::vector<uint8_t> kinds;
};

bool read_words(FILE *fp, size_t n, std::vector<uint64_t> &dst) {
    unsigned long long x;
    for (size_t j = 0; j < n; j++) {
        if (fscanf(fp, "%llu", &x) != 1) return false;
        dst.push_back(x);
    }
    return true;
}

bool read_proofs(const char *path, std::vector<Proof> &out) {
    FILE *fp = fopen(path, "r");
    if (!fp) return false;
    unsigned long long d, v, rev, cfe, c, f, kind;
    bool ok = true;
    while (ok && fscanf(fp, "%llu %llu %llu %llu %llu %llu", &d, &v, &rev, &cfe, &c, &f) == 6) {
        if (d < 1 || d > pv::MAX_DEGREE || v < 1 || v > 32) {
            ok = false;
            break;
        }
        Proof p;
        p.d = (unsigned)d;
        p.v = v;
        p.reversed = rev != 0;
        p.check_fe = cfe != 0;
        p.claimed = c;
        p.final_eval = f;
        ok = read_words(fp, (d + 1) * v, p.rounds) && read_words(fp, v, p.point) && read_words(fp, d, p.fevals);
        for (unsigned j = 0; ok && j < d; j++) {
            ok = fscanf(fp, "%llu", &kind) == 1 && kind <= 1;
            p.kinds.push_back((uint8_t)kind);
            if (ok) ok = kind ? read_words(fp, v, p.taus) : read_words(fp, 1, p.table_evals);
        }
        if (ok) out.push_back(p);
    }
    fclose(fp);
    return ok;
}

// the oracles of one proof: a table's evaluation as given, an eq factor's in closed form
void oracles(const Proof &p, uint64_t *ev) {
    size_t t = 0, e = 0;
    for (unsigned j = 0; j < p.d; j++)
        ev[j] = p.kinds[j] ? pv::eq_at(p.taus.data() + p.v * e++, p.point.data(), p.v, p.reversed) : p.table_evals[t++];
}

int verify(const char *path) {
    std::vector<Proof> proofs;
    if (!read_proofs(path, proofs)) return 2;
    alignas(16) static uint32_t dummy[4];  // the tables are not read by the device form's checks
    for (const Proof &p : proofs) {
        const size_t n = (size_t)1 << p.v;
        const void *factors[pv::MAX_DEGREE];
        for (unsigned j = 0; j < p.d; j++) factors[j] = p.kinds[j] ? nullptr : dummy;
        size_t rejected = 0, bad = UNTOUCHED;
        const pv::VerifyArgs a{1, &p.d, factors, p.kinds.data(), p.taus.empty() ? nullptr : p.taus.data(), &n, &p.claimed, p.rounds.data(),
                               p.point.data(), p.check_fe ? p.fevals.data() : nullptr, &p.final_eval,
                               p.reversed ? ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED : 0u, &rejected};
        const zigz_status st = pv::check_verify_product_batch(a, true, false, &bad);
        if (st != ZIGZ_OK) {
            printf("check failed: status %d at %lld\n", (int)st, (long long)bad);
            return 1;
        }
        const sv::Replay r = pv::replay_rounds(p.claimed, p.rounds.data(), p.v, p.d);
        uint64_t ev[pv::MAX_DEGREE];
        oracles(p, ev);
        printf("%d %d %llu", (int)pv::verdict(r, ev, p.d, p.final_eval, p.check_fe ? p.fevals.data() : nullptr), r.rounds_ok ? 1 : 0,
               (unsigned long long)r.expected);
        for (unsigned j = 0; j < p.d; j++) printf(" %llu", (unsigned long long)ev[j]);
        if (p.d == 1) {
            const sv::Replay lin = sv::replay_rounds(p.claimed, p.rounds.data(), p.v);
            printf(" %d", lin.rounds_ok == r.rounds_ok && lin.expected == r.expected ? 1 : 0);
        }
        printf("\n");
    }
    return 0;
}

int time_replay(const char *path, int reps) {
    std::vector<Proof> proofs;
    if (!read_proofs(path, proofs) || reps < 1) return 2;
    const size_t k = proofs.size();
    std::vector<sv::Replay> rep(k);
    std::vector<uint64_t> ev(k * pv::MAX_DEGREE);
    std::vector<double> ms;
    for (int r = -2; r < reps; r++) {  // two warm-ups
        const auto t0 = std::chrono::steady_clock::now();
        parallel_for(k, [&](size_t i) {
            const Proof &p = proofs[i];
            rep[i] = pv::replay_rounds(p.claimed, p.rounds.data(), p.v, p.d);
            oracles(p, ev.data() + i * pv::MAX_DEGREE);
        });
        const std::chrono::duration<double, std::milli> d = std::chrono::steady_clock::now() - t0;
        if (r >= 0) ms.push_back(d.count());
    }
    std::sort(ms.begin(), ms.end());
    size_t ok = 0;
    for (const auto &r : rep) ok += r.rounds_ok;
    printf("replay_ms %.4f %.4f %.4f %zu\n", ms[ms.size() / 2], ms.front(), ms.back(), ok);
    return 0;
}

// four proofs of degrees 1, 3, 2, 3 over n = 2, 8, 4, 16; proofs 1 and 3 have eq(tau, .) as their first factor
struct Batch {
    std::vector<std::vector<uint64_t>> tables;
    std::vector<const void *> host, dev;
    std::vector<unsigned> degrees;
    std::vector<uint8_t> kinds;
    std::vector<size_t> ns;
    std::vector<uint64_t> claimed, finals, rounds, points, fevals, taus;
    std::vector<uint64_t *> eq_out;
    std::vector<uint32_t *> eq_dev;
    std::vector<std::vector<uint64_t>> eq_host;
    Batch() {
        alignas(16) static uint32_t dummy[8];
        const size_t nn[4] = {2, 8, 4, 16};
        const unsigned dd[4] = {1, 3, 2, 3};
        for (int i = 0; i < 4; i++) {
            ns.push_back(nn[i]);
            degrees.push_back(dd[i]);
            const size_t v = log2_floor(nn[i]);
            for (unsigned j = 0; j < dd[i]; j++) {
                const bool eq = (i == 1 || i == 3) && j == 0;
                kinds.push_back(eq ? 1 : 0);
                tables.emplace_back(nn[i], 5);
                fevals.push_back(9 + j);
                if (eq)
                    for (size_t x = 0; x < v; x++) taus.push_back(21 + x);
            }
            for (size_t x = 0; x < v; x++) {
                points.push_back(7 + x);
                for (unsigned j = 0; j <= dd[i]; j++) rounds.push_back(11 + x + j);
            }
            claimed.push_back(3);
            finals.push_back(4);
            eq_host.emplace_back(nn[i], 0);
        }
        for (size_t f = 0; f < tables.size(); f++) {
            host.push_back(kinds[f] ? nullptr : tables[f].data());
            dev.push_back(kinds[f] ? nullptr : dummy);
        }
        for (auto &e : eq_host) {
            eq_out.push_back(e.data());
            eq_dev.push_back(dummy);
        }
    }
    size_t voff(size_t i) const {
        size_t o = 0;
        for (size_t j = 0; j < i; j++) o += log2_floor(ns[j]);
        return o;
    }
    size_t roff(size_t i) const {
        size_t o = 0;
        for (size_t j = 0; j < i; j++) o += (degrees[j] + 1) * log2_floor(ns[j]);
        return o;
    }
    size_t foff(size_t i) const {
        size_t o = 0;
        for (size_t j = 0; j < i; j++) o += degrees[j];
        return o;
    }
};

void report(const char *name, zigz_status st, size_t bad) { printf("%s %d %lld\n", name, (int)st, (long long)bad); }

struct Opt {
    uint32_t flags = 0;
    bool rejected = true, kinds = true, taus = true, fevals = true;
};
void verify_case(const char *name, const Batch &b, size_t k, bool dev, const Opt &o = Opt()) {
    size_t bad = UNTOUCHED, rejected = 77;
    const pv::VerifyArgs a{k, b.degrees.data(), dev ? b.dev.data() : b.host.data(), o.kinds ? b.kinds.data() : nullptr,
                           o.taus ? b.taus.data() : nullptr, b.ns.data(), b.claimed.data(), b.rounds.data(), b.points.data(),
                           o.fevals ? b.fevals.data() : nullptr, b.finals.data(), o.flags, o.rejected ? &rejected : nullptr};
    const zigz_status st = dev ? pv::check_verify_product_batch(a, true, false, &bad) : pv::check_verify_product_batch_host(a, &bad);
    report(name, st, bad);
}
void eq_case(const char *name, const Batch &b, size_t k, bool dev, bool with_points = true) {
    size_t bad = UNTOUCHED;
    const zigz_status st = pv::check_eq_table_batch(k, b.ns.data(), with_points ? b.points.data() : nullptr,
                                                    dev ? (const void *const *)b.eq_dev.data() : (const void *const *)b.eq_out.data(), dev, &bad);
    report(name, st, bad);
}

int check() {
    const uint64_t p = ZIGZ_BABYBEAR_P;
    const Batch good;
    const size_t k = good.ns.size();
    for (int dev = 0; dev < 2; dev++) {
        const char *s = dev ? "dev" : "host";
        char name[64];
#define CASE(fmt) (snprintf(name, sizeof name, fmt "_%s", s), name)
        eq_case(CASE("eq_ok"), good, k, dev);
        eq_case(CASE("eq_k0"), good, 0, dev);
        eq_case(CASE("eq_k4097"), good, 4097, dev);
        eq_case(CASE("eq_no_points"), good, k, dev, false);
        verify_case(CASE("verify_ok"), good, k, dev);
        {
            Opt o;
            o.flags = ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED;
            verify_case(CASE("verify_reversed_ok"), good, k, dev, o);
            o.flags = 2;
            verify_case(CASE("verify_flag2"), good, k, dev, o);
        }
        verify_case(CASE("verify_k0"), good, 0, dev);
        verify_case(CASE("verify_k4097"), good, 4097, dev);
        {
            Opt o;
            o.rejected = false;
            verify_case(CASE("verify_no_rejected"), good, k, dev, o);
        }
        {
            Opt o;
            o.fevals = false;
            verify_case(CASE("verify_no_fevals_ok"), good, k, dev, o);
        }
        {  // kinds NULL: every factor is a table, and proof 1's first pointer is NULL
            Opt o;
            o.kinds = false;
            verify_case(CASE("verify_no_kinds_null1"), good, k, dev, o);
        }
        {  // an eq factor without eq_points: proof 1
            Opt o;
            o.taus = false;
            verify_case(CASE("verify_no_taus1"), good, k, dev, o);
        }
        // shapes: entry 1 gets n = 0, 1, 3, 2^33 (the words of the entries behind it are still in bounds: fewer variables, or
        // the call stops there)
        for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)1 << 33}) {
            Batch b;
            b.ns[1] = n;
            snprintf(name, sizeof name, "eq_n%zu_%s", n, s);
            eq_case(name, b, k, dev);
            snprintf(name, sizeof name, "verify_n%zu_%s", n, s);
            if (n <= 3) verify_case(name, b, k, dev);  // (2^33: the rounds of a 33-variable proof are not there to be read)
        }
        {
            Batch b;
            b.degrees[2] = 0;
            verify_case(CASE("verify_degree0_2"), b, 3, dev);
            b.degrees[2] = 4;
            verify_case(CASE("verify_degree4_2"), b, 3, dev);
        }
        {
            Batch b;
            b.kinds[b.foff(2) + 1] = 2;
            verify_case(CASE("verify_kind2_2"), b, k, dev);
        }
        {  // an eq factor with a table pointer
            Batch b;
            b.host[b.foff(3)] = b.tables[0].data();
            b.dev[b.foff(3)] = b.dev[b.foff(3) + 1];
            verify_case(CASE("verify_eq_with_pointer3"), b, k, dev);
        }
        {  // a word >= p in each array, at a proof of its own
            Batch b;
            b.points[b.voff(3) + 2] = p;
            eq_case(CASE("eq_point3"), b, k, dev);
            verify_case(CASE("verify_point3"), b, k, dev);
        }
        {
            Batch b;
            b.rounds[b.roff(1) + 5] = p + 5;
            verify_case(CASE("verify_round1"), b, k, dev);
            eq_case(CASE("eq_ignores_rounds"), b, k, dev);
        }
        {
            Batch b;
            b.claimed[2] = ~0ull;
            verify_case(CASE("verify_claimed2"), b, k, dev);
        }
        {
            Batch b;
            b.finals[0] = p;
            verify_case(CASE("verify_final0"), b, k, dev);
        }
        {
            Batch b;
            b.fevals[b.foff(2) + 1] = p;
            verify_case(CASE("verify_feval2"), b, k, dev);
            Opt o;
            o.fevals = false;
            verify_case(CASE("verify_feval2_unread"), b, k, dev, o);
        }
        {  // proof 3's tau: its words come after proof 1's three
            Batch b;
            b.taus[3 + 1] = p;
            verify_case(CASE("verify_tau3"), b, k, dev);
        }
        {  // the first failing proof wins: proof 1's point before proof 2's final eval; a word >= p before a later shape error
            Batch b;
            b.finals[2] = p;
            b.points[b.voff(1)] = p;
            verify_case(CASE("verify_first_of_two"), b, k, dev);
            Batch c;
            c.ns[3] = 12;
            c.rounds[b.roff(2)] = p;
            verify_case(CASE("verify_round2_before_n12_3"), c, k, dev);
            Batch e;
            e.ns[2] = 3;
            e.taus[4] = p;
            verify_case(CASE("verify_n3_2_before_tau3"), e, k, dev);
        }
        {  // p - 1 is canonical
            Batch b;
            b.finals[0] = b.claimed[1] = b.points[0] = b.rounds[0] = b.taus[0] = b.fevals[0] = p - 1;
            verify_case(CASE("verify_p_minus_1"), b, k, dev);
        }
#undef CASE
    }
    {  // host tables: a value >= p in front of a later shape error is reported instead; behind it, it is not
        Batch b;
        b.tables[b.foff(1) + 2][3] = p;
        b.ns[3] = 12;
        verify_case("verify_value1_before_n12_3_host", b, k, false);
        Batch c;
        c.tables[c.foff(3) + 1][0] = p;
        c.ns[2] = 3;
        verify_case("verify_n3_2_before_value3_host", c, k, false);
        Batch e;  // (an eq factor's unused table is never read)
        e.tables[e.foff(1)][0] = p;
        e.ns[3] = 12;
        verify_case("verify_eq_slot_unread_host", e, k, false);
    }
    {  // outputs and device tables: null and misaligned pointers
        Batch b;
        b.eq_out[3] = nullptr;
        eq_case("eq_null3_host", b, k, false);
        b.eq_dev[1] = b.eq_dev[1] + 1;
        eq_case("eq_misaligned1_dev", b, k, true);
        b.eq_dev[0] = nullptr;
        eq_case("eq_null0_dev", b, k, true);
        Batch c;
        c.dev[c.foff(2) + 1] = (const uint8_t *)c.dev[c.foff(2) + 1] + 4;
        verify_case("verify_misaligned2_dev", c, k, true);
        c.dev[0] = nullptr;
        verify_case("verify_null0_dev", c, k, true);
        c.host[0] = nullptr;
        verify_case("verify_null0_host", c, k, false);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "verify")) return verify(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 4 && !strcmp(argv[1], "time")) return time_replay(argv[2], atoi(argv[3]));
    fprintf(stderr, "usage: %s verify FILE | check | time FILE REPS\n", argv[0]);
    return 2;
}
