// Stand-alone driver of zigz_amd/csrc/sumcheck_verify_host.hpp (no GPU, no HIP): built with -fsanitize=address,undefined by
// tests/test_sumcheck_verify_cpu.py and run as a child process.
//   replay FILE   FILE holds one proof per line: v claimed_sum final_eval, then 2 v round coefficients and v point coordinates.
//                 Runs the argument checker over the whole batch (must pass), then prints per proof "rounds_ok expected_eval".
//   time FILE R   the replays of FILE's proofs on the library's host threads (host_parallel.hpp), R times after a warm-up: prints
//                 "replay_ms median min max rounds_ok" (tools/mle_eval_batch_rate.py: the host's replay alone)
//   check         runs the argument checkers on bad shapes and prints "case status bad_index" per case (bad_index -1: untouched).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "host_parallel.hpp"
#include "sumcheck_verify_host.hpp"

using namespace zk;

namespace {

const size_t UNTOUCHED = (size_t)-1;

struct Proofs {
    std::vector<size_t> ns, voff;
    std::vector<uint64_t> claimed, finals, rounds, points;
};

bool read_proofs(const char *path, Proofs &p) {
    FILE *fp = fopen(path, "r");
    if (!fp) return false;
    unsigned long long v, c, f, x;
    p.voff.push_back(0);
    while (fscanf(fp, "%llu %llu %llu", &v, &c, &f) == 3) {
        if (v < 1 || v > 32) return false;
        p.ns.push_back((size_t)1 << v);
        p.voff.push_back(p.voff.back() + v);
        p.claimed.push_back(c);
        p.finals.push_back(f);
        for (unsigned long long j = 0; j < 2 * v; j++) {
            if (fscanf(fp, "%llu", &x) != 1) return false;
            p.rounds.push_back(x);
        }
        for (unsigned long long j = 0; j < v; j++) {
            if (fscanf(fp, "%llu", &x) != 1) return false;
            p.points.push_back(x);
        }
    }
    fclose(fp);
    return true;
}

int replay(const char *path) {
    Proofs p;
    if (!read_proofs(path, p)) return 2;
    const size_t k = p.ns.size();
    // the tables are not read by the device form's checks: any aligned non-null address will do
    alignas(16) static uint32_t dummy[4];
    std::vector<const void *> tabs(k, dummy);
    size_t rejected = 0, bad = UNTOUCHED;
    const zigz_status st = sv::check_verify_batch(tabs.data(), p.ns.data(), k, p.claimed.data(), p.rounds.data(), p.points.data(),
                                                  p.finals.data(), 0, &rejected, true, false, &bad);
    if (st != ZIGZ_OK) {
        printf("check failed: status %d at %lld\n", (int)st, (long long)bad);
        return 1;
    }
    for (size_t i = 0; i < k; i++) {
        const sv::Replay r = sv::replay_rounds(p.claimed[i], p.rounds.data() + 2 * p.voff[i], p.voff[i + 1] - p.voff[i]);
        printf("%d %llu\n", r.rounds_ok ? 1 : 0, (unsigned long long)r.expected);
    }
    return 0;
}

// the k replays as the verify entries run them (parallel_for's threads), timed alone: "replay_ms median min max accepted"
int time_replay(const char *path, int reps) {
    Proofs p;
    if (!read_proofs(path, p) || reps < 1) return 2;
    const size_t k = p.ns.size();
    std::vector<sv::Replay> rep(k);
    std::vector<double> ms;
    for (int r = -2; r < reps; r++) {  // two warm-ups
        const auto t0 = std::chrono::steady_clock::now();
        parallel_for(k, [&](size_t i) { rep[i] = sv::replay_rounds(p.claimed[i], p.rounds.data() + 2 * p.voff[i], p.voff[i + 1] - p.voff[i]); });
        const std::chrono::duration<double, std::milli> d = std::chrono::steady_clock::now() - t0;
        if (r >= 0) ms.push_back(d.count());
    }
    std::sort(ms.begin(), ms.end());
    size_t ok = 0;
    for (const auto &r : rep) ok += r.rounds_ok;
    printf("replay_ms %.4f %.4f %.4f %zu\n", ms[ms.size() / 2], ms.front(), ms.back(), ok);
    return 0;
}

struct Batch {
    std::vector<std::vector<uint64_t>> tables;
    std::vector<const void *> host, dev;
    std::vector<size_t> ns;
    std::vector<uint64_t> claimed, finals, rounds, points, out;
    Batch() {
        alignas(16) static uint32_t dummy[8];
        for (size_t n : {2, 8, 4, 16}) {
            ns.push_back(n);
            tables.emplace_back(n, 5);
            for (size_t j = 0; j < log2_floor(n); j++) {
                points.push_back(7 + j);
                rounds.push_back(11 + j);
                rounds.push_back(13 + j);
            }
            claimed.push_back(3);
            finals.push_back(4);
        }
        for (auto &t : tables) {
            host.push_back(t.data());
            dev.push_back(dummy);
        }
        out.assign(ns.size(), 0);
    }
    size_t off(size_t i) const {
        size_t o = 0;
        for (size_t j = 0; j < i; j++) o += log2_floor(ns[j]);
        return o;
    }
};

void report(const char *name, zigz_status st, size_t bad) { printf("%s %d %lld\n", name, (int)st, (long long)bad); }

void eval_case(const char *name, const Batch &b, size_t k, bool dev) {
    size_t bad = UNTOUCHED;
    const zigz_status st =
        sv::check_eval_batch(dev ? b.dev.data() : b.host.data(), b.ns.data(), k, b.points.data(), b.out.data(), dev, true, &bad);
    report(name, st, bad);
}
void verify_case(const char *name, const Batch &b, size_t k, bool dev, uint32_t flags = 0, bool with_rejected = true) {
    size_t bad = UNTOUCHED, rejected = 77;
    const zigz_status st =
        sv::check_verify_batch(dev ? b.dev.data() : b.host.data(), b.ns.data(), k, b.claimed.data(), b.rounds.data(), b.points.data(),
                               b.finals.data(), flags, with_rejected ? &rejected : nullptr, dev, true, &bad);
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
        eval_case(CASE("eval_ok"), good, k, dev);
        eval_case(CASE("eval_k0"), good, 0, dev);
        eval_case(CASE("eval_k4097"), good, 4097, dev);
        verify_case(CASE("verify_ok"), good, k, dev);
        verify_case(CASE("verify_reversed_ok"), good, k, dev, ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED);
        verify_case(CASE("verify_k0"), good, 0, dev);
        verify_case(CASE("verify_k4097"), good, 4097, dev);
        verify_case(CASE("verify_flag2"), good, k, dev, 2);
        verify_case(CASE("verify_no_rejected"), good, k, dev, 0, false);
        // shapes: pair 1 gets n = 0, 1, 3 (the points of the pairs behind it are still in bounds: fewer variables)
        for (size_t n : {0, 1, 3}) {
            Batch b;
            b.ns[1] = n;
            snprintf(name, sizeof name, "eval_n%zu_%s", n, s);
            eval_case(name, b, k, dev);
            snprintf(name, sizeof name, "verify_n%zu_%s", n, s);
            verify_case(name, b, k, dev);
        }
        {  // a word >= p in each array, at a pair of its own
            Batch b;
            b.points[b.off(3) + 2] = p;
            eval_case(CASE("eval_point3"), b, k, dev);
            verify_case(CASE("verify_point3"), b, k, dev);
        }
        {
            Batch b;
            b.rounds[2 * b.off(1) + 3] = p + 5;
            verify_case(CASE("verify_round1"), b, k, dev);
            eval_case(CASE("eval_ignores_rounds"), b, k, dev);
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
        {  // the first failing pair wins: pair 1's point before pair 2's final eval
            Batch b;
            b.finals[2] = p;
            b.points[b.off(1)] = p;
            verify_case(CASE("verify_first_of_two"), b, k, dev);
        }
        {  // p - 1 is canonical
            Batch b;
            b.finals[0] = b.claimed[1] = b.points[0] = b.rounds[0] = p - 1;
            verify_case(CASE("verify_p_minus_1"), b, k, dev);
        }
#undef CASE
    }
    {  // host tables: a value >= p; device tables: a null and a misaligned pointer
        Batch b;
        b.tables[2][3] = p;
        eval_case("eval_value2_host", b, k, false);
        verify_case("verify_value2_host", b, k, false);
        b.tables[2][3] = 5;
        b.host[3] = nullptr;
        eval_case("eval_null3_host", b, k, false);
        b.dev[1] = (const uint8_t *)b.dev[1] + 4;
        eval_case("eval_misaligned1_dev", b, k, true);
        verify_case("verify_misaligned1_dev", b, k, true);
        b.dev[0] = nullptr;
        eval_case("eval_null0_dev", b, k, true);
        verify_case("verify_null0_dev", b, k, true);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "replay")) return replay(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 4 && !strcmp(argv[1], "time")) return time_replay(argv[2], atoi(argv[3]));
    fprintf(stderr, "usage: %s replay FILE | check | time FILE REPS\n", argv[0]);
    return 2;
}
