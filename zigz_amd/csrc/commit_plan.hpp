#pragma once
// The host side of a commit job's build (api_commit.cpp), pure host code with no HIP in it so that it can be exercised without a
// GPU (tests/c_driver/commit_plan_host.cpp): where the storage of the structure-aware levels goes (ONE list of regions, placed
// by the single build in its workspaces and by the batched build in its arenas), what the words of a build's summary mean, how a
// proof's summary turns into statistics, and what a context learns from it about the room its next builds' lists need.
#include <stddef.h>
#include <stdint.h>

#include "zigz_hip.h"

namespace zk {
namespace cp {

constexpr unsigned MAX_LEVELS = 20;  // = RUN_MAX_LEVELS (kernels.hpp; api_commit.cpp asserts it)

// ------------------------------------------------------------------ storage of the list-built levels
// R (run-aware columns): the list of hashed nodes and the stages' scratch; kept while the trees are read: bitmap | prev | woff
// (runs_meta_words entries each), ubase (runs_units entries), the digests in list order.  G (content-addressed group): the
// table (keys: generation-tagged, FIRST of its regions -- a build finds the table of the one before at the same place), its
// slots' list positions and the list; kept: every node's representative and the digests in list order.  UPPER: the levels
// above the lists, of all columns.
enum Region { R_LIST, R_STAGE, R_BITMAP, R_PREV, R_WOFF, R_UBASE, R_STORE, G_KEYS, G_IDX, G_LIST, G_REP, G_STORE, UPPER, N_REGIONS };
constexpr unsigned bit(Region r) { return 1u << r; }
constexpr unsigned R_SCRATCH = bit(R_LIST) | bit(R_STAGE);
constexpr unsigned R_KEPT = bit(R_BITMAP) | bit(R_PREV) | bit(R_WOFF) | bit(R_UBASE) | bit(R_STORE);
constexpr unsigned G_SCRATCH = bit(G_KEYS) | bit(G_IDX) | bit(G_LIST);
constexpr unsigned G_KEPT = bit(G_REP) | bit(G_STORE);
constexpr unsigned ALL_REGIONS = (1u << N_REGIONS) - 1;

// what the sizes depend on (runs_lists / cons_lists: entries; runs_meta_words, runs_units, runs_stage_scratch_bytes: kernels.hpp)
struct Shape {
    size_t npad, rn, gn, ncols;  // leaves; R, G and all columns
    uint64_t r_entries, g_entries;
    size_t meta_words, units, stage_bytes;
};
// Where a build's regions are: the single build spreads them over workspaces (scratch apart from what its openings read, so
// that a proof in flight holds no more than it needs), the batched build puts everything into its arena (space 0).
enum Space { SP_RUNS, SP_RUNMETA, SP_CONS, SP_CONSMETA, SP_UPPER, N_SPACES };
struct Plan {
    size_t bytes[N_REGIONS];  // 0: the build has no such region (no R / no G columns)
    size_t off[N_REGIONS];    // in its space
    unsigned char space[N_REGIONS];
    size_t total[N_SPACES];   // bytes of every space
};
// (the 64 bytes behind the lists, the stage scratch, ubase and the stores are slack the single build always gave them)
inline Plan region_sizes(const Shape &s) {
    Plan p{};
    if (s.rn) {
        p.bytes[R_LIST] = (size_t)s.r_entries * 4;
        p.bytes[R_STAGE] = s.stage_bytes + 64;
        p.bytes[R_BITMAP] = s.meta_words * 8;
        p.bytes[R_PREV] = p.bytes[R_WOFF] = s.meta_words * 2;
        p.bytes[R_UBASE] = s.units * 4 + 64;
        p.bytes[R_STORE] = (size_t)s.r_entries * 32 + 64;
    }
    if (s.gn) {
        p.bytes[G_KEYS] = 2 * s.npad * 8;
        p.bytes[G_IDX] = p.bytes[G_REP] = 2 * s.npad * 4;
        p.bytes[G_LIST] = (size_t)s.g_entries * 4 + 64;
        p.bytes[G_STORE] = (size_t)s.g_entries * s.gn * 32 + 64;
    }
    p.bytes[UPPER] = s.ncols * 512 * 32;
    return p;
}
// appends the regions of `mask` (those the build has) to space sp, each aligned to `align` (a power of two), as is the end
inline void place(Plan &p, Space sp, unsigned mask, size_t align) {
    size_t at = p.total[sp];
    for (unsigned r = 0; r < N_REGIONS; r++)
        if (((mask >> r) & 1) && p.bytes[r]) {
            at = (at + align - 1) & ~(align - 1);
            p.off[r] = at;
            p.space[r] = (unsigned char)sp;
            at += p.bytes[r];
        }
    p.total[sp] = (at + align - 1) & ~(align - 1);
}
// A single build.  A commit job keeps what its openings read (and the upper levels) in spaces of their own, which nothing but
// the next job touches; any other build puts it behind its scratch and the upper levels into a space shared with other calls.
inline Plan plan_single(const Shape &s, bool job) {
    Plan p = region_sizes(s);
    place(p, SP_RUNS, R_SCRATCH, 64);
    place(p, job ? SP_RUNMETA : SP_RUNS, R_KEPT, 64);
    place(p, SP_CONS, G_SCRATCH, 64);  // (the table at offset 0)
    place(p, job ? SP_CONSMETA : SP_CONS, G_KEPT, 64);
    place(p, !job ? SP_UPPER : s.rn ? SP_RUNMETA : SP_CONSMETA, bit(UPPER), 64);
    return p;
}
// One proof's arena of a batched build: everything behind the `head` bytes of its columns and counters; total[0] is where its
// slabs go.
inline Plan plan_arena(const Shape &s, size_t head) {
    Plan p = region_sizes(s);
    p.total[0] = head;
    place(p, SP_RUNS, ALL_REGIONS, 256);
    return p;
}

// ------------------------------------------------------------------ a build's summary
// The words k_job_summary writes behind a job's roots, per proof (kernels.hpp: JOB_SUMMARY_WORDS of them):
enum SummaryWord {
    SUM_R_HASHED = 0,    // nodes hashed on the run-aware levels
    SUM_SD_WAVES = 1,    // waves of the small-domain columns that left the tables ...
    SUM_G_SD_WAVES = 2,  // ... and of a dropped group's small-domain members
    SUM_G_HASHED = 3,    // digests computed on the content-addressed levels
    SUM_G_DROPPED = 4,   // != 0: the group did not repeat and was dropped on the device
    SUM_G_DISTINCT = 5,  // its distinct leaves
    SUM_FLAGS = 6,       // FLAG_* below
    SUM_R_CONSTANT = 7,  // run-aware columns found constant
    SUM_R_LONGEST = 8,   // + level: the longest sub-list of the R lists ...
    SUM_G_LONGEST = 8 + MAX_LEVELS,  // ... and of the G lists
    SUMMARY_WORDS = 8 + 2 * MAX_LEVELS
};
constexpr unsigned long long FLAG_R_OVER = 1, FLAG_G_OVER = 1 << 8, FLAG_G_NO_SLABS = 2 << 8;

// what a job's build asked for (the same for every proof of a batched job; an arena build has sd_cols = cons_sd = 0)
struct JobFacts {
    uint64_t run_cols, run_dense;  // R columns; their nodes on the list levels
    uint64_t sd_cols;              // small-domain columns (levels 0 and 1 from the tables)
    uint64_t cons_hinted, cons_levels_nodes, cons_sd;  // the group's columns; nodes per column on the list levels; its small-domain members
    uint64_t perms0;               // permutations of the dense build, less the small-domain columns' table levels
    uint64_t N;
};
// Adds one proof, whose summary words are h, to the build fields of the stats.
inline void tally_add(zigz_kernel_stats &t, const unsigned long long *h, const JobFacts &f) {
    // the run-aware levels hashed h[SUM_R_HASHED] of their run_dense nodes
    const uint64_t r_hashed = f.run_cols ? h[SUM_R_HASHED] : 0;
    t.run_aware_dense_nodes += f.run_dense;
    t.run_aware_hashed += r_hashed;
    t.eval_constant_columns += f.run_cols ? h[SUM_R_CONSTANT] : 0;
    t.small_domain_columns += f.sd_cols;
    t.small_domain_fallback_waves += f.sd_cols ? h[SUM_SD_WAVES] : 0;
    t.list_hash_perms += r_hashed;
    t.keccak_permutations += f.perms0 - (f.run_dense - r_hashed);
    if (!f.cons_hinted) return;
    // the group: kept (digests computed for its cons_dense_nodes nodes) or dropped on the device (its small-domain members then
    // took levels 0 and 1 from the tables, everything else was hashed densely by the level launches)
    const uint64_t dense = f.cons_hinted * f.cons_levels_nodes, table_levels = f.cons_sd * (f.N + f.N / 2);
    t.cons_probe_distinct += h[SUM_G_DISTINCT];
    if (!h[SUM_G_DROPPED]) {
        t.cons_columns = f.cons_hinted;  // (the hinted count if any proof kept its group)
        t.cons_dense_nodes += dense;
        t.cons_hashed += h[SUM_G_HASHED];
        t.keccak_permutations -= dense - h[SUM_G_HASHED];
        t.list_hash_perms += h[SUM_G_HASHED];
    } else {
        t.small_domain_columns += f.cons_sd;
        t.small_domain_fallback_waves += h[SUM_G_SD_WAVES];
        t.keccak_permutations -= table_levels;
        t.list_hash_perms += dense - table_levels;
    }
}
// The build fields of a job's stats: the sums over its nz proofs' summaries (a single job is one proof).  Returns the job's
// constant columns (what its eval leaves out).
inline uint64_t job_stats(zigz_kernel_stats &t, const unsigned long long *h, unsigned nz, const JobFacts &f) {
    t.run_aware_columns = f.run_cols;
    t.run_aware_dense_nodes = t.run_aware_hashed = t.eval_constant_columns = t.small_domain_columns = t.small_domain_fallback_waves = 0;
    t.list_hash_perms = t.keccak_permutations = t.cons_probe_distinct = t.cons_columns = t.cons_dense_nodes = t.cons_hashed = 0;
    for (unsigned z = 0; z < nz; z++) tally_add(t, h + (size_t)z * SUMMARY_WORDS, f);
    return t.eval_constant_columns;
}

// ------------------------------------------------------------------ the room of the lists, learnt
// How much room the lists (and the digests stored in list order) of the structure-aware levels get: learnt from what the
// context's previous builds of the same shape needed, not sized for the worst case.
struct ListCaps {
    size_t npad;
    unsigned rn, gn;
    unsigned r[MAX_LEVELS], g[MAX_LEVELS];  // entries per sub-list and level
    bool g_slabs;  // this context's traces made the group be dropped: give its columns slabs up front
    unsigned g_drops, g_skip;  // consecutive builds that dropped the group; builds left that do not even try it
    unsigned g_kept;           // consecutive builds that kept it (from the second on the probe pass is left out)
    unsigned r_last[MAX_LEVELS], g_last[MAX_LEVELS];  // the longest sub-list of the LAST build per level (0: none yet): launch sizing only
    bool last_dropped;  // ... and whether it dropped its group (whose columns are then hashed densely by the level launches)
};
// the last list-built level of a tree of N leaves (run_top_level): 256 nodes per column
inline unsigned top_level(uint64_t N) { unsigned v = 0; while (((uint64_t)1 << v) < N) v++; return v - 8; }
// What the lists of a single job's build (with lists) needed: the context remembers it for its next builds.  Returns whether
// the build has to be repeated with the new room: a list ran out of it, or the group was dropped with nowhere to build its
// columns densely.  Caps of another shape learn nothing.
inline bool learn_caps(ListCaps &c, const unsigned long long *h, const JobFacts &f) {
    if (c.npad != f.N) return false;
    const unsigned long long flags = h[SUM_FLAGS];
    const bool r_over = (flags & FLAG_R_OVER) != 0, g_over = (flags & FLAG_G_OVER) != 0, g_noslab = (flags & FLAG_G_NO_SLABS) != 0;
    const bool dropped = h[SUM_G_DROPPED] != 0, g_on = f.cons_hinted && !dropped;
    for (unsigned l = 0; l <= top_level(f.N); l++) {
        const unsigned long long ru = h[SUM_R_LONGEST + l], gu = h[SUM_G_LONGEST + l];
        c.r_last[l] = f.run_cols ? (unsigned)(ru ? ru : 1) : 0;
        c.g_last[l] = g_on ? (unsigned)(gu ? gu : 1) : 0;
        if (f.run_cols && (r_over ? ru > c.r[l] : ru * 10 > (unsigned long long)c.r[l] * 8)) c.r[l] = (unsigned)(ru + ru / 4 + 64);
        if (g_on && (g_over ? gu > c.g[l] : gu * 10 > (unsigned long long)c.g[l] * 8)) c.g[l] = (unsigned)(gu + gu / 4 + 64);
        // A G list that ran out of room hides what the levels above it need: the nodes that found no slot share their
        // sub-list's last one, so their parents' keys look alike and the level above counts too few.  Learning one level
        // per build would take more builds than a job may repeat: give every level at least the room of the one below
        // (the lists never get more than "every node hashed", cons_lists).
        if (g_over && g_on && l > 0 && c.g[l] < c.g[l - 1]) c.g[l] = c.g[l - 1];
    }
    c.last_dropped = dropped;
    if (dropped) c.g_slabs = true;  // this context's traces do not repeat: give the group's columns slabs from now on
    if (f.cons_hinted) {
        c.g_drops = dropped ? c.g_drops + 1 : 0;
        c.g_kept = dropped ? 0 : c.g_kept + 1;
        // ... and after the second drop in a row, skip the attempt for 15 jobs -- twice as many after every further attempt
        // that is dropped again (a context shared by a service's lanes sees hundreds of jobs of one kind of trace)
        if (c.g_drops >= 2) c.g_skip = 15u << (c.g_drops - 2 < 6 ? c.g_drops - 2 : 6);
    }
    return r_over || (g_over && !dropped) || g_noslab;
}

}  // namespace cp
}  // namespace zk
