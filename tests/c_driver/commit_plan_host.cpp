// The host side of a commit job's build (zigz_amd/csrc/commit_plan.hpp) without a GPU: prints, for the inputs of a text file,
// where the three builds place the storage of the list-built levels, what a job's summaries tally to, and what a context
// learns from a sequence of them.  tests/test_commit_plan_cpu.py writes the inputs and checks what comes back.
// Usage: commit_plan_host layout|tally|learn FILE
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "commit_plan.hpp"

using namespace zk::cp;

static std::vector<unsigned long long> numbers(const std::string &line) {
    std::istringstream in(line);
    std::vector<unsigned long long> v;
    for (unsigned long long x; in >> x;) v.push_back(x);
    return v;
}
static JobFacts facts(const unsigned long long *v) { return JobFacts{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}; }

static void print_plan(const char *name, const Plan &p) {
    printf("%s", name);
    for (unsigned r = 0; r < N_REGIONS; r++) printf(" %u:%zu:%zu", (unsigned)p.space[r], p.off[r], p.bytes[r]);
    printf(" |");
    for (unsigned sp = 0; sp < N_SPACES; sp++) printf(" %zu", p.total[sp]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[2]);
    std::string line;
    if (!strcmp(argv[1], "layout")) {  // npad rn gn ncols r_entries g_entries meta_words units stage_bytes head
        while (std::getline(in, line)) {
            const std::vector<unsigned long long> v = numbers(line);
            if (v.size() != 10) return 2;
            const Shape s{(size_t)v[0], (size_t)v[1], (size_t)v[2], (size_t)v[3], v[4], v[5], (size_t)v[6], (size_t)v[7], (size_t)v[8]};
            print_plan("job", plan_single(s, true));
            print_plan("other", plan_single(s, false));
            print_plan("arena", plan_arena(s, (size_t)v[9]));
        }
    } else if (!strcmp(argv[1], "tally")) {  // nz, the 8 facts, nz x SUMMARY_WORDS words
        while (std::getline(in, line)) {
            const std::vector<unsigned long long> v = numbers(line);
            if (v.size() < 9 || v.size() != 9 + v[0] * SUMMARY_WORDS) return 2;
            const JobFacts f = facts(&v[1]);
            zigz_kernel_stats t;
            memset(&t, 0xA5, sizeof(t));  // (whatever the last job left)
            job_stats(t, &v[9], (unsigned)v[0], f);
            const uint64_t got[] = {t.run_aware_columns, t.run_aware_dense_nodes, t.run_aware_hashed, t.small_domain_columns,
                                    t.small_domain_fallback_waves, t.cons_columns, t.cons_dense_nodes, t.cons_hashed, t.cons_probe_distinct,
                                    t.list_hash_perms, t.keccak_permutations, t.eval_constant_columns};
            for (uint64_t x : got) printf("%llu ", (unsigned long long)x);
            printf("\n");
        }
    } else if (!strcmp(argv[1], "learn")) {  // first line: npad, r[], g[], g_slabs g_drops g_skip g_kept last_dropped; then facts + words
        if (!std::getline(in, line)) return 2;
        std::vector<unsigned long long> v = numbers(line);
        if (v.size() != 1 + 2 * MAX_LEVELS + 5) return 2;
        ListCaps c{};
        c.npad = (size_t)v[0];
        for (unsigned l = 0; l < MAX_LEVELS; l++) {
            c.r[l] = (unsigned)v[1 + l];
            c.g[l] = (unsigned)v[1 + MAX_LEVELS + l];
        }
        const unsigned long long *q = &v[1 + 2 * MAX_LEVELS];
        c.g_slabs = q[0] != 0;
        c.g_drops = (unsigned)q[1];
        c.g_skip = (unsigned)q[2];
        c.g_kept = (unsigned)q[3];
        c.last_dropped = q[4] != 0;
        while (std::getline(in, line)) {
            v = numbers(line);
            if (v.size() != 8 + SUMMARY_WORDS) return 2;
            const bool again = learn_caps(c, &v[8], facts(&v[0]));
            printf("%d", (int)again);
            for (const unsigned *a : {c.r, c.g, c.r_last, c.g_last})
                for (unsigned l = 0; l < MAX_LEVELS; l++) printf(" %u", a[l]);
            printf(" %d %u %u %u %d\n", (int)c.g_slabs, c.g_drops, c.g_skip, c.g_kept, (int)c.last_dropped);
        }
    } else {
        return 2;
    }
    return 0;
}
