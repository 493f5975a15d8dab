// Stand-alone driver of the radix schedules and the tail rounds of zigz_amd/csrc/sumcheck_host.hpp (no GPU, no HIP): built with
// -fsanitize=address,undefined, and once more with -fsanitize=thread, by tests/test_radix_host_cpu.py and run as a child process.
// The data passes are plain C++ over std::vector tables; the ranks of a sharded run are threads, their all-gather a barrier over a
// shared buffer.  Tables come from a seed (splitmix64 mod p, tests/oracle_lib.py: splitmix64_field) or a pattern: seed 1 = all
// p - 1, seed 2 = low half 0, high half p - 1.  Outputs start as a sentinel, so what a run did not write shows.
//   radix_host FILE   one command per line of FILE:
//     run WORLD N_LOCAL SEED FIXED_SEED BAD_ROUND GLOBAL FAIL_RANK FAIL_OP
//         radix_run of the table of WORLD * N_LOCAL values, rank r holding the values r, r + WORLD, ...  FIXED_SEED != 0: fixed
//         challenges from that seed, of which challenge BAD_ROUND (>= 0) is p.  GLOBAL: the passes add the block sums over the
//         ranks themselves (sums_global).  FAIL_RANK >= 0: that rank's fold (FAIL_OP 1) or read_tail (2) returns ZIGZ_ERR_HIP.
//         Prints per rank: "run RANK STATUS ERR ALLGATHERS : 2 v rounds : v point : final_eval" (ERR: 0 none, 1 the hook failed,
//         2 another rank reported an error).
//     batch FIXED_SEED FAIL K N_0 SEED_0 ... N_{K-1} SEED_{K-1}
//         radix_run_batch; FAIL: the fold pass returns ZIGZ_ERR_HIP.  Prints "batch STATUS", then per table
//         "table I : rounds : point : final_eval".
//     tail N SEED
//         the N <= 1024 values through SumcheckRounds::tail_rounds at one factor and through the linear tail written out here
//         (half sums, one subtraction per round); prints "tail STATUS : rounds : point : final_eval" for each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sumcheck_host.hpp"

using namespace zk;

namespace {

const uint64_t SENTINEL = 0xA5A5A5A5A5A5A5A5ull;
const uint64_t P = ZIGZ_BABYBEAR_P;

std::vector<uint64_t> table(uint64_t seed, size_t n) {
    std::vector<uint64_t> t(n);
    for (size_t i = 0; i < n; i++) {
        if (seed == 1) { t[i] = P - 1; continue; }
        if (seed == 2) { t[i] = i < n / 2 ? 0 : P - 1; continue; }
        uint64_t z = seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        t[i] = (z ^ (z >> 31)) % P;
    }
    return t;
}

void print_words(const std::vector<uint64_t> &rounds, const std::vector<uint64_t> &point, uint64_t fe) {
    printf(" :");
    for (uint64_t x : rounds) printf(" %llu", (unsigned long long)x);
    printf(" :");
    for (uint64_t x : point) printf(" %llu", (unsigned long long)x);
    printf(" : %llu\n", (unsigned long long)fe);
}

// ---- the data passes of one table
std::vector<uint64_t> block_sums_of(const std::vector<uint64_t> &t, unsigned k) {
    const size_t nb = (size_t)1 << k, m = t.size() >> k;
    std::vector<uint64_t> s(nb, 0);
    for (size_t b = 0; b < nb; b++)
        for (size_t i = 0; i < m; i++) s[b] += t[b * m + i];
    return s;
}
std::vector<uint64_t> fold_of(const std::vector<uint64_t> &t, unsigned k, const uint64_t *w) {
    const size_t nb = (size_t)1 << k, m = t.size() >> k;
    std::vector<uint64_t> out(m, 0);
    for (size_t b = 0; b < nb; b++) {
        if (w[b] >= P) abort();  // canonical weights
        for (size_t i = 0; i < m; i++) out[i] = f_add(out[i], f_mul(w[b], t[b * m + i]));
    }
    return out;
}

// ---- the ranks of one run
struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    size_t world, waiting = 0, generation = 0;
    void wait() {
        std::unique_lock<std::mutex> lock(mu);
        const size_t g = generation;
        if (++waiting == world) {
            waiting = 0;
            generation++;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != g; });
        }
    }
};
struct Shared {
    Barrier barrier;
    std::vector<uint8_t> buf;  // world slots of `slot` bytes
    size_t slot;
};
struct Rank {
    Shared *sh;
    size_t rank, world;
    std::vector<uint64_t> cur;
    bool global;
    int fail_op;  // 1: fold fails, 2: read_tail fails
    size_t allgathers = 0;
    zigz_status st = ZIGZ_OK;
    const char *err = nullptr;
    std::vector<uint64_t> rounds, point;
    uint64_t fe = SENTINEL;

    // every rank's n words -> all of them on every rank
    void gather(const void *send, size_t bytes, void *recv) {
        if (bytes > sh->slot) abort();
        memcpy(sh->buf.data() + rank * sh->slot, send, bytes);
        sh->barrier.wait();
        for (size_t r = 0; r < world; r++) memcpy((uint8_t *)recv + r * bytes, sh->buf.data() + r * sh->slot, bytes);
        sh->barrier.wait();
    }
    void reduce(uint64_t *sums, size_t n) {  // the stand-in for a collective inside the pass
        if (!global || world == 1) return;
        std::vector<uint64_t> all(world * n);
        gather(sums, n * 8, all.data());
        for (size_t i = 0; i < n; i++) {
            sums[i] = 0;
            for (size_t r = 0; r < world; r++) sums[i] += all[r * n + i];
        }
    }
};

int rank_allgather(void *user, const void *send, size_t bytes, void *recv) {
    Rank *r = (Rank *)user;
    r->allgathers++;
    r->gather(send, bytes, recv);
    return 0;
}
zigz_status rank_block_sums(void *user, unsigned k, uint64_t *sums) {
    Rank *r = (Rank *)user;
    const std::vector<uint64_t> s = block_sums_of(r->cur, k);
    memcpy(sums, s.data(), s.size() * 8);
    r->reduce(sums, s.size());
    return ZIGZ_OK;
}
zigz_status rank_fold(void *user, unsigned k, const uint64_t *weights, unsigned k_next, uint64_t *next_sums) {
    Rank *r = (Rank *)user;
    if (r->fail_op == 1) return ZIGZ_ERR_HIP;
    r->cur = fold_of(r->cur, k, weights);
    if (k_next) {
        const std::vector<uint64_t> s = block_sums_of(r->cur, k_next);
        memcpy(next_sums, s.data(), s.size() * 8);
        r->reduce(next_sums, s.size());
    } else if (next_sums) {
        abort();
    }
    return ZIGZ_OK;
}
zigz_status rank_read_tail(void *user, size_t m, uint64_t *out) {
    Rank *r = (Rank *)user;
    if (r->fail_op == 2) return ZIGZ_ERR_HIP;
    if (m != r->cur.size()) return ZIGZ_ERR_PROTOCOL_ERROR;
    memcpy(out, r->cur.data(), m * 8);
    return ZIGZ_OK;
}

int run(size_t world, size_t n_local, uint64_t seed, uint64_t fixed_seed, long bad_round, bool global, long fail_rank, int fail_op) {
    const std::vector<uint64_t> t = table(seed, world * n_local);
    const size_t nv = log2_floor(world * n_local);
    std::vector<uint64_t> fixed;
    if (fixed_seed) {
        fixed = table(fixed_seed, nv);
        if (bad_round >= 0) fixed[(size_t)bad_round] = P;
    }
    if (shard_check(n_local, 0, (int)world, true) != ZIGZ_OK) return 2;
    Shared sh;
    sh.barrier.world = world;
    sh.slot = (n_local + 1024 + 8) * 8;
    sh.buf.assign(world * sh.slot, 0);
    std::vector<Rank> ranks(world);
    for (size_t r = 0; r < world; r++) {
        Rank &k = ranks[r];
        k.sh = &sh;
        k.rank = r;
        k.world = world;
        k.global = global;
        k.fail_op = (long)r == fail_rank ? fail_op : 0;
        for (size_t j = 0; j < n_local; j++) k.cur.push_back(t[j * world + r]);
        k.rounds.assign(2 * nv, SENTINEL);
        k.point.assign(nv, SENTINEL);
    }
    auto prove = [&](size_t r) {
        Rank &k = ranks[r];
        const RadixOps ops{&k, rank_block_sums, rank_fold, rank_read_tail};
        const ShardComm comm{(int)r, (int)world, rank_allgather, &k, global};
        k.st = radix_run(ops, n_local, &comm, fixed.empty() ? nullptr : fixed.data(), k.rounds.data(), k.point.data(), &k.fe, &k.err);
    };
    std::vector<std::thread> th;
    for (size_t r = 1; r < world; r++) th.emplace_back(prove, r);
    prove(0);
    for (auto &x : th) x.join();
    for (const Rank &k : ranks) {
        const int err = !k.err ? 0 : !strcmp(k.err, "sharded sumcheck: the all-gather hook failed") ? 1
                        : !strcmp(k.err, "sharded sumcheck: another rank reported an error")    ? 2
                                                                                                : 3;
        printf("run %zu %d %d %zu", k.rank, (int)k.st, err, k.allgathers);
        print_words(k.rounds, k.point, k.fe);
    }
    return 0;
}

// ---- the passes of a batch
struct Batch {
    std::vector<std::vector<uint64_t>> cur;
    bool fail;
};
zigz_status batch_block_sums(void *user, size_t count, const size_t *tables, const unsigned *ks, uint64_t *sums) {
    Batch *b = (Batch *)user;
    for (size_t j = 0; j < count; j++) {
        const std::vector<uint64_t> s = block_sums_of(b->cur[tables[j]], ks[j]);
        memcpy(sums, s.data(), s.size() * 8);
        sums += s.size();
    }
    return ZIGZ_OK;
}
zigz_status batch_fold(void *user, size_t count, const size_t *tables, const unsigned *ks, const uint64_t *weights,
                       const unsigned *knext, uint64_t *next_sums) {
    Batch *b = (Batch *)user;
    if (b->fail) return ZIGZ_ERR_HIP;
    for (size_t j = 0; j < count; j++) {
        std::vector<uint64_t> &t = b->cur[tables[j]];
        t = fold_of(t, ks[j], weights);
        weights += (size_t)1 << ks[j];
        if (!knext[j]) continue;
        const std::vector<uint64_t> s = block_sums_of(t, knext[j]);
        memcpy(next_sums, s.data(), s.size() * 8);
        next_sums += s.size();
    }
    return ZIGZ_OK;
}
zigz_status batch_read_tail(void *user, size_t count, const size_t *tables, const size_t *ms, uint64_t *out) {
    Batch *b = (Batch *)user;
    for (size_t j = 0; j < count; j++) {
        const std::vector<uint64_t> &t = b->cur[tables[j]];
        if (ms[j] != t.size()) return ZIGZ_ERR_PROTOCOL_ERROR;
        memcpy(out, t.data(), t.size() * 8);
        out += t.size();
    }
    return ZIGZ_OK;
}

int batch(uint64_t fixed_seed, bool fail, const std::vector<size_t> &ns, const std::vector<uint64_t> &seeds) {
    const size_t k = ns.size();
    Batch b;
    b.fail = fail;
    std::vector<size_t> voff(k + 1, 0);
    for (size_t i = 0; i < k; i++) {
        if (mle_check(ns[i]) != ZIGZ_OK || ns[i] < 2) return 2;
        b.cur.push_back(table(seeds[i], ns[i]));
        voff[i + 1] = voff[i] + log2_floor(ns[i]);
    }
    std::vector<uint64_t> fixed, rounds(2 * voff[k], SENTINEL), points(voff[k], SENTINEL), fe(k, SENTINEL);
    if (fixed_seed) fixed = table(fixed_seed, voff[k]);
    const zigz_status st = radix_run_batch(BatchOps{&b, batch_block_sums, batch_fold, batch_read_tail}, k, ns.data(),
                                           fixed.empty() ? nullptr : fixed.data(), rounds.data(), points.data(), fe.data());
    printf("batch %d\n", (int)st);
    for (size_t i = 0; i < k; i++) {
        printf("table %zu", i);
        print_words(std::vector<uint64_t>(rounds.begin() + 2 * voff[i], rounds.begin() + 2 * voff[i + 1]),
                    std::vector<uint64_t>(points.begin() + voff[i], points.begin() + voff[i + 1]), fe[i]);
    }
    return 0;
}

// ---- the tail rounds at one factor against the linear tail written out
int tail(size_t n, uint64_t seed) {
    if (mle_check(n) != ZIGZ_OK || n < 2 || n > HOST_TAIL_MAX) return 2;
    const size_t nv = log2_floor(n);
    {
        std::vector<uint64_t> t = table(seed, n), rounds(2 * nv, SENTINEL), point(nv, SENTINEL);
        SumcheckRounds s;
        s.nv = nv;
        s.rounds = rounds.data();
        s.point = point.data();
        const uint64_t fe = s.tail_rounds(&t);
        printf("tail %d", (int)s.st);
        print_words(rounds, point, fe);
    }
    {
        std::vector<uint64_t> t = table(seed, n), rounds, point;
        Transcript tr;
        while (t.size() > 1) {
            const size_t half = t.size() / 2;
            uint64_t s0 = 0, s1 = 0;
            for (size_t x = 0; x < half; x++) {
                s0 = (s0 + t[x]) % P;
                s1 = (s1 + t[x + half]) % P;
            }
            const uint64_t c[2] = {s0, (s1 + P - s0) % P};
            tr.append_field(c[0]);
            tr.append_field(c[1]);
            const uint64_t ch = tr.challenge();
            rounds.insert(rounds.end(), c, c + 2);
            point.push_back(ch);
            for (size_t x = 0; x < half; x++) t[x] = (t[x] + (uint64_t)(((unsigned __int128)ch * ((t[x + half] + P - t[x]) % P)) % P)) % P;
            t.resize(half);
        }
        printf("tail %d", (int)ZIGZ_OK);
        print_words(rounds, point, t[0]);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: radix_host FILE\n");
        return 2;
    }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) return 2;
    char cmd[16];
    int rc = 0;
    while (rc == 0 && fscanf(fp, "%15s", cmd) == 1) {
        if (!strcmp(cmd, "run")) {
            unsigned long long world, n_local, seed, fixed_seed;
            long bad_round, fail_rank;
            int global, fail_op;
            if (fscanf(fp, "%llu %llu %llu %llu %ld %d %ld %d", &world, &n_local, &seed, &fixed_seed, &bad_round, &global, &fail_rank,
                       &fail_op) != 8)
                rc = 2;
            else
                rc = run(world, n_local, seed, fixed_seed, bad_round, global != 0, fail_rank, fail_op);
        } else if (!strcmp(cmd, "batch")) {
            unsigned long long fixed_seed, k, n, seed;
            int fail;
            std::vector<size_t> ns;
            std::vector<uint64_t> seeds;
            if (fscanf(fp, "%llu %d %llu", &fixed_seed, &fail, &k) != 3) rc = 2;
            for (unsigned long long i = 0; rc == 0 && i < k; i++) {
                if (fscanf(fp, "%llu %llu", &n, &seed) != 2) rc = 2;
                ns.push_back(n);
                seeds.push_back(seed);
            }
            if (rc == 0) rc = batch(fixed_seed, fail != 0, ns, seeds);
        } else if (!strcmp(cmd, "tail")) {
            unsigned long long n, seed;
            rc = fscanf(fp, "%llu %llu", &n, &seed) == 2 ? tail(n, seed) : 2;
        } else {
            rc = 2;
        }
    }
    fclose(fp);
    return rc;
}
