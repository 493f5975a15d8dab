// C ABI of libzigz_hip.so, part 3: Merkle trees (dense and structure-aware builds), the commitment scheme and the commit jobs of
// Prover.generateCommitments (single and batched).
#include "api_internal.hpp"

using namespace zk;
using cp::ListCaps;
static_assert(cp::MAX_LEVELS == RUN_MAX_LEVELS && cp::SUMMARY_WORDS == JOB_SUMMARY_WORDS, "commit_plan.hpp restates kernels.hpp");

// ------------------------------------------------------------------ Merkle
// How much room the lists (and the digests stored in list order) of the structure-aware levels get: learnt from what the
// context's previous builds needed, not sized for the worst case -- a build that runs out says so and is repeated with more
// (zigz_commit_roots), which costs one extra build the first time a context meets a new kind of trace.
static void caps_for(zigz_ctx *ctx, size_t npad, unsigned rn, unsigned gn) {
    ListCaps &c = ctx->caps;
    if (c.npad == npad && c.rn == rn && c.gn == gn) return;
    c.npad = npad;
    c.rn = rn;
    c.gn = gn;
    c.g_slabs = false;
    c.g_drops = c.g_skip = c.g_kept = 0;
    memset(c.r_last, 0, sizeof(c.r_last));
    memset(c.g_last, 0, sizeof(c.g_last));
    c.last_dropped = false;
    const LevelLists rw = runs_lists(npad, rn ? rn : 1), gw = cons_lists(npad);
    for (unsigned l = 0; l < RUN_MAX_LEVELS; l++) {
        c.r[l] = l <= rw.top ? (rw.cap[l] / 8 > 256 ? rw.cap[l] / 8 : 256) : 0;  // an eighth of "every node hashed"
        c.g[l] = l <= gw.top ? 256 : 0;                                           // 8192 distinct nodes per level
    }
}

// A TreeRef without any storage yet: no column has a slab, is run-aware or member of the group.
static TreeRef empty_tree_ref(size_t npad) {
    TreeRef t{};
    t.npad = npad;
    memset(t.slab_of_col, -1, sizeof(t.slab_of_col));
    memset(t.y_of_col, -1, sizeof(t.y_of_col));
    memset(t.g_j_of_col, -1, sizeof(t.g_j_of_col));
    return t;
}
// nodes per column on the list-built levels 0 .. top
static uint64_t list_level_nodes(size_t npad) {
    uint64_t n = 0;
    for (unsigned l = 0; l <= run_top_level(npad); l++) n += npad >> l;
    return n;
}
// The list-built levels of the R and G columns of a build of `ncols` columns: fills what t says about them (r_caps / g_caps:
// room per sub-list, nullptr = the worst case) and returns what the sizes of their storage depend on (commit_plan.hpp).
static cp::Shape tree_ref_lists(TreeRef &t, const ColMap &R, const ColMap &G, size_t ncols, const unsigned *r_caps, const unsigned *g_caps) {
    const size_t npad = t.npad;
    cp::Shape s{npad, R.n, G.n, ncols, 0, 0, 0, 0, 0};
    t.lists = 1;
    t.top = run_top_level(npad);
    if (R.n) {
        t.r_lists = runs_lists(npad, R.n, r_caps);
        s.units = runs_units(npad, R.n, t.ubase_off);
        s.r_entries = t.r_lists.entries;
        s.meta_words = runs_meta_words(npad, R.n);
        s.stage_bytes = runs_stage_scratch_bytes(npad, R.n);
        t.ncols = R.n;
        for (unsigned y = 0; y < R.n; y++) t.y_of_col[R.c[y]] = (signed char)y;
    }
    if (G.n) {
        t.g_lists = cons_lists(npad, g_caps);
        s.g_entries = t.g_lists.entries;
        t.g_ncols = G.n;
        for (unsigned k = 0; k < G.n; k++) t.g_j_of_col[G.c[k]] = (signed char)k;
    }
    return s;
}
// ... and the pointers into that storage, region r of the plan at base[space of r] + its offset (g_ctr: the build's G counters)
static void point_at_regions(MerkleBuild &b, TreeRef &t, const cp::Plan &p, uint8_t *const base[cp::N_SPACES], unsigned long long *g_ctr) {
    auto at = [&](cp::Region r) { return base[p.space[r]] + p.off[r]; };
    t.upper = at(cp::UPPER);
    if (b.rcols.n) {
        b.r_list = (uint32_t *)at(cp::R_LIST);
        b.r_stage = at(cp::R_STAGE);
        t.bitmap = (unsigned long long *)at(cp::R_BITMAP);
        t.prev = (unsigned short *)at(cp::R_PREV);
        t.woff = (unsigned short *)at(cp::R_WOFF);
        t.ubase = (uint32_t *)at(cp::R_UBASE);
        t.r_store = at(cp::R_STORE);
    }
    if (b.gcols.n) {
        b.g_keys = (unsigned long long *)at(cp::G_KEYS);
        b.g_idx = (uint32_t *)at(cp::G_IDX);
        b.g_list = (uint32_t *)at(cp::G_LIST);
        b.g_rep = (uint32_t *)at(cp::G_REP);
        t.g_rep = b.g_rep;
        t.g_store = at(cp::G_STORE);
        b.g_ctr = g_ctr;
        t.g_dropped = g_ctr + 8;
    }
}

// Builds all levels of `ncols` trees, asynchronously on the stream.
// in.job (a commit job's build): the digests of the list-built levels stay in list order (TreeRef: stores), only densely
//   built columns get node-addressed slabs (taken from WS_TREE); out->tree describes where everything is and stays valid while
//   the context's WS_RUNMETA / WS_CONSMETA / WS_TREE workspaces are untouched -- until the job ends.
// !in.job, or in.materialize: every digest of every tree is written into node-addressed slabs (d_slab if given: single trees
//   that outlive the call; else WS_TREE), one per column.
zigz_status build_trees(zigz_ctx *ctx, const uint32_t *d_vals, size_t val_stride, size_t n_values, size_t npad,
                               uint8_t *d_slab, size_t ncols, bool record, const BuildHints &in, BuildResult *out) {
    const unsigned height = log2_floor(npad);
    const size_t stride = tree_nodes(npad);
    const bool job = in.job;
    *out = BuildResult{};
    if (record) ctx->kev_n = 0;
    // the list counters of a commit job's build are read again by its openings (EvalSkip, the "group dropped" word): they are
    // the job's; any other build on the context counts in the auxiliary pair
    unsigned long long *const r_ctr = job ? ctx->d_run_count : ctx->d_run_aux, *const g_ctr = job ? ctx->d_cons_count : ctx->d_cons_aux;
    // timing mode: every launch (or bracketed group of launches) carries its own begin / end timestamps, by class
    KTime kt_store;
    auto stamp = [&](int cls, uint64_t perms) -> const KTime * {
        if (!record || ctx->kev_n >= KEV_MAX) return nullptr;
        kt_store = KTime{ctx->kev[2 * ctx->kev_n], ctx->kev[2 * ctx->kev_n + 1]};
        ctx->kev_class[ctx->kev_n] = (uint8_t)cls;
        ctx->kev_perms[ctx->kev_n] = perms;
        ctx->kev_n++;
        return &kt_store;
    };
    // Four kinds of columns:
    //   G  hinted as a group that repeats in the same places (the columns that are functions of the instruction at pc): the
    //      levels 0 .. v - 8 are content-addressed -- takes precedence over H and R.  Whether the group repeats enough to be
    //      worth it is decided ON THE DEVICE after the leaf level's table pass (more than a quarter of the leaves distinct:
    //      dropped); a dropped group's columns are built like H (its small-domain members) and D (the rest) by launches that
    //      read the same device flag, so nothing here waits for the device;
    //   H  hinted small-domain (values < 128 by construction): levels 0 and 1 from two constant tables, checked per wave
    //      and hashed where the bound does not hold;
    //   R  hinted run-aware (piecewise constant): the levels 0 .. v - 8 from lists of the nodes that are not a copy of their
    //      left neighbour -- decided from the values, so the hint cannot make a tree wrong;
    //   D  the rest: hashed densely.
    // The top kernel (256 nodes per column -> root) takes all columns together.
    ColMap H{}, R{}, D{}, G{}, GS{};
    const bool big = npad >= RUN_MIN_LEAVES && npad <= RUN_MAX_LEAVES && ncols <= 64;
    const bool sd_ok = in.small_domain_mask && npad >= 1024 && ncols <= 64 && val_stride % 2 == 0 && ((uintptr_t)d_vals & 7) == 0;
    const bool run_ok = in.run_aware_mask && big;
    // (a content-addressing key packs two child list slots into RUN_NODE_BITS bits each, and a slot is sub-list * capacity +
    // position: at npad == 2^26 a nearly full last sub-list reaches 2^26 + 2047 -- the group path stops one size short of that)
    bool cons_ok = in.cons_group_mask && big && npad < RUN_MAX_LEAVES;
    unsigned gn_hinted = 0;  // (what the context learnt is filed under the hints, not under whether this build tries the group)
    for (size_t c = 0; cons_ok && c < ncols; c++) gn_hinted += (unsigned)((in.cons_group_mask >> c) & 1);
    if (run_ok || cons_ok) {
        unsigned rn_hinted = 0;
        for (size_t c = 0; run_ok && c < ncols; c++)
            rn_hinted += (unsigned)(((in.run_aware_mask >> c) & 1) && !(cons_ok && ((in.cons_group_mask >> c) & 1)) &&
                                    !(sd_ok && ((in.small_domain_mask >> c) & 1)));
        caps_for(ctx, npad, rn_hinted, gn_hinted);
    }
    // A context whose last two jobs dropped the group (its traces do not loop) stops trying for a while: the group's columns
    // are then H / D from the start -- no table passes that find nothing, and the tuned dense kernels instead of the list
    // kernel's dense branch -- and every 16th job looks again.
    if (cons_ok && job && !ctx->cons_always && ctx->caps.npad == npad && ctx->caps.g_skip) {
        ctx->caps.g_skip--;
        cons_ok = false;
    }
    auto kind = [&](size_t c) -> int {  // 0 D, 1 H, 2 R, 3 G
        if (cons_ok && ((in.cons_group_mask >> c) & 1)) return 3;
        if (sd_ok && ((in.small_domain_mask >> c) & 1)) return 1;
        if (run_ok && ((in.run_aware_mask >> c) & 1)) return 2;
        return 0;
    };
    if (sd_ok || run_ok || cons_ok)
        for (size_t c = 0; c < ncols; c++) {
            const int kd = kind(c);
            ColMap &m = kd == 3 ? G : kd == 1 ? H : kd == 2 ? R : D;
            m.c[m.n++] = (uint8_t)c;
            if (kd == 3 && sd_ok && ((in.small_domain_mask >> c) & 1)) GS.c[GS.n++] = (uint8_t)c;
        }
    const bool lists = R.n || G.n;
    const bool whole = !job || in.materialize;  // every digest into node-addressed slabs
    const bool virt = !whole;  // copies / non-representatives / table leaves never written
    // ---- where the digests go
    TreeRef t = empty_tree_ref(npad);
    size_t nslab = 0;
    if (whole || !lists) {
        nslab = ncols;
        for (size_t c = 0; c < ncols && c < 64; c++) t.slab_of_col[c] = (signed char)c;
    } else {
        for (size_t c = 0; c < ncols; c++) {
            const int kd = kind(c);
            if (kd == 0 || kd == 1 || (kd == 3 && ctx->caps.g_slabs)) t.slab_of_col[c] = (signed char)nslab++;
        }
    }
    if (d_slab) t.slab = d_slab;  // (a single tree: ncols slabs of the caller's)
    else if (nslab) {
        void *w;
        CHK(ws_get(ctx, WS_TREE, nslab * stride * 32, &w));
        t.slab = (uint8_t *)w;
    }
    auto slab_map = [&](const ColMap &m) {  // for the dense kernels: entry k of m -> its slab
        ColMap o{};
        o.n = m.n;
        for (unsigned k = 0; k < m.n; k++) o.c[k] = (uint8_t)t.slab_of_col[m.c[k]];
        return o;
    };
    if (H.n == 0 && R.n == 0 && G.n == 0) {
        launch_keccak_leaves(d_vals, val_stride, n_values, npad, t.slab, stride, ncols, ctx->stream, stamp(0, (uint64_t)ncols * npad));
    } else if (D.n) {
        const ColMap ds = slab_map(D);
        launch_keccak_leaves(d_vals, val_stride, n_values, npad, t.slab, stride, ncols, ctx->stream, stamp(0, (uint64_t)D.n * npad), &D, &ds);
    }
    void *sd_todo = nullptr;
    if (H.n || GS.n) {
        if (!ctx->d_sd_tables) {
            HIPCHK(ctx, hipMalloc((void **)&ctx->d_sd_tables, SD_TABLE_BYTES));
            HIPCHK(ctx, hipMalloc((void **)&ctx->d_sd_fallbacks, 64));
            launch_sd_tables(ctx->d_sd_tables, ctx->stream);
        }
        CHK(ws_get(ctx, WS_DEDUP, (sd_todo_words(npad, H.n) + sd_todo_words(npad, GS.n)) * 4, &sd_todo));
    }
    // every counter this build's kernels add to, zeroed by ONE launch (three memsets are three commands in the stream)
    if (H.n || GS.n || R.n || G.n)
        launch_zero_counters((H.n || GS.n) ? ctx->d_sd_fallbacks : nullptr, R.n ? r_ctr : nullptr,
                             G.n ? g_ctr : nullptr, ctx->stream);
    if (H.n) {
        // in a commit job the leaf digests of these columns are left out (virtual): only an opening reads one, and it
        // hashes that value itself
        const ColMap hs = slab_map(H);
        launch_keccak_small_l01(d_vals, val_stride, n_values, npad, t.slab, stride, H, ctx->d_sd_tables, ctx->d_sd_fallbacks,
                                (uint32_t *)sd_todo, ctx->stream, stamp(3, 0), !virt, nullptr, &hs);
        if (virt)
            for (unsigned k = 0; k < H.n; k++) t.virtual_leaves |= 1ull << H.c[k];
        out->sd_cols = H.n;
    }
    MerkleBuild b{};
    unsigned top = 0;
    if (lists) {
        // what outlives the build (read by the openings): a commit job keeps it in workspaces of its own, which nothing but
        // the next commit job touches; otherwise it is scratch like the rest (cp::plan_single).  Only a commit job can repeat
        // a build that ran out of room: anything else gets the worst case.
        const cp::Shape shape = tree_ref_lists(t, R, G, ncols, job ? ctx->caps.r : nullptr, job ? ctx->caps.g : nullptr);
        const cp::Plan plan = cp::plan_single(shape, job);
        static const int slot[cp::N_SPACES] = {WS_RUNS, WS_RUNMETA, WS_CONS, WS_CONSMETA, WS_OUT64};
        uint8_t *base[cp::N_SPACES] = {};
        for (int sp = 0; sp < cp::N_SPACES; sp++) {
            void *w = nullptr;
            if (plan.total[sp]) CHK(ws_get(ctx, slot[sp], plan.total[sp], &w));
            base[sp] = (uint8_t *)w;
        }
        top = t.top;
        b.vals = d_vals;
        b.val_stride = val_stride;
        b.n_values = n_values;
        b.npad = npad;
        b.rcols = R;
        b.gcols = G;
        b.gcols_sd = GS;
        point_at_regions(b, t, plan, base, g_ctr);
        if (R.n) {
            b.r_ctr = r_ctr;
            out->run_cols = R.n;
            out->run_dense = (uint64_t)R.n * list_level_nodes(npad);
        }
        if (G.n) {
            // the table (generation-tagged, at offset 0 of its workspace): cleared only when the workspace is new or the
            // generations run out
            void *const w = base[cp::SP_CONS];
            if (ctx->cons_table != w || ctx->cons_table_bytes != ctx->ws_bytes[WS_CONS] || ctx->cons_gen + RUN_MAX_LEVELS + 1 >= 4096) {
                HIPCHK(ctx, hipMemsetAsync(w, 0, plan.bytes[cp::G_KEYS], ctx->stream));  // generation 0 = free
                ctx->cons_table = w;
                ctx->cons_table_bytes = ctx->ws_bytes[WS_CONS];
                ctx->cons_gen = 1;
            }
            b.g_gen = ctx->cons_gen;
            ctx->cons_gen += top + 1;
            b.g_has_slabs = whole || ctx->caps.g_slabs;
            static const bool always_probe = getenv("ZIGZ_CONS_PROBE_ALWAYS") != nullptr;  // (A/B)
            b.g_no_probe = job && ctx->caps.npad == npad && ctx->caps.g_kept >= 2 && !ctx->cons_always && !always_probe;
            if (virt)
                for (unsigned k = 0; k < GS.n; k++) t.g_sd_mask |= 1ull << GS.c[k];
            out->cons_hinted = G.n;
            out->cons_levels_nodes = list_level_nodes(npad);
            out->cons_sd = GS.n;
        }
        b.t = t;
        if (ctx->debug_skip != 2) launch_structure(b, ctx->stream, ctx->debug_skip == 0, stamp(4, 0));
        if (GS.n && b.g_has_slabs) {  // only if the group was dropped: its small-domain members' levels 0 and 1 by table
            const ColMap gs = slab_map(GS);
            launch_keccak_small_l01(d_vals, val_stride, n_values, npad, t.slab, stride, GS, ctx->d_sd_tables, ctx->d_sd_fallbacks + 1,
                                    (uint32_t *)sd_todo + sd_todo_words(npad, H.n), ctx->stream, stamp(3, 0), !virt, g_ctr + 8,
                                    &gs);
        }
    }
    out->tree = t;
    unsigned first_top = 0;  // the level the top kernel starts from
    if (lists) {
        for (unsigned l = 0; l <= top; l++) {
            size_t expect = 0;  // what the last build of this shape held here, + 25 % + the sub-lists' slack (sizing only)
            if (job && ctx->caps.npad == npad && (ctx->caps.r_last[l] || ctx->caps.g_last[l])) {
                auto more = [](unsigned v) { return (size_t)RUN_SUBS * (v + v / 4 + 8); };
                expect = (R.n ? more(ctx->caps.r_last[l]) : 0) + (G.n ? more(ctx->caps.g_last[l]) * G.n : 0) +
                         (G.n && ctx->caps.last_dropped ? (size_t)G.n * (npad >> l) : 0);
            }
            if (ctx->debug_skip != 1) launch_level_hash(b, l, ctx->stream, stamp(5, 0), expect, ctx->debug_skip == 0);
            if (l == top) break;
            ColMap m{};  // the densely built columns that already have level l: D, and H from level 1
            for (size_t c = 0; c < ncols; c++) {
                const int kd = kind(c);
                if (kd == 0 || (kd == 1 && l >= 1)) m.c[m.n++] = (uint8_t)c;
            }
            if (m.n) {
                const ColMap ms = slab_map(m);
                launch_keccak_level(t.slab, stride, tree_level_offset(npad, l), tree_level_offset(npad, l + 1), npad >> (l + 1), ncols,
                                    ctx->stream, stamp(keccak_level_is_wide(npad >> (l + 1), m.n) ? 1 : 2, (uint64_t)m.n * (npad >> (l + 1))), &ms);
            }
        }
        first_top = top;
    } else {
        for (unsigned l = 0; l < height; l++) {  // level l + 1 from level l, for the columns that do not have it yet
            const size_t n_out = npad >> (l + 1);
            first_top = l;
            if (n_out <= 256) break;  // all columns are complete here (H stops at level 1): the top kernel takes over
            ColMap m{};
            const ColMap *pm = nullptr;
            size_t nc = ncols;
            if (H.n && l < 1) {  // the table columns join at level 1
                for (size_t c = 0; c < ncols; c++)
                    if (kind(c) == 0) m.c[m.n++] = (uint8_t)c;
                if (m.n == 0) continue;
                pm = &m;
                nc = m.n;
            }
            launch_keccak_level(t.slab, stride, tree_level_offset(npad, l), tree_level_offset(npad, l + 1), n_out, ncols, ctx->stream,
                                stamp(keccak_level_is_wide(n_out, nc) ? 1 : 2, (uint64_t)nc * n_out), pm);
        }
    }
    if (height) {
        if (ctx->debug_skip != 1) launch_merkle_top(t, first_top, height, ncols, ctx->stream, stamp(6, (uint64_t)ncols * ((npad >> first_top) - 1)));
    }
    if (lists && whole) launch_fill_virtual(b, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return ZIGZ_OK;
}

// after the stream has passed the last recorded launch: per-class device time of the last recorded build
zigz_status keccak_times_collect(zigz_ctx *ctx) {
    // 0 leaves, 1 wide levels, 2 small levels, 3 small-domain table lookups, 4 structure passes (run-aware stages + content-
    // addressing table passes: no hashing), 5 list-driven level hashing, 6 the top of the trees
    double us[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t perms[7] = {0, 0, 0, 0, 0, 0, 0};
    ctx->log_n = 0;
    for (int i = 0; i < ctx->kev_n; i++) {
        double d = 0;
        HIPCHK(ctx, hipEventSynchronize(ctx->kev[2 * i + 1]));
        CHK(log_launch(ctx, ctx->kev_class[i], ctx->kev_perms[i], ctx->kev[2 * i], ctx->kev[2 * i + 1], ctx->kev[0], &d));
        us[ctx->kev_class[i]] += d;
        perms[ctx->kev_class[i]] += ctx->kev_perms[i];
    }
    ctx->stats.keccak_leaves_us = us[0];
    ctx->stats.keccak_leaves_perms = perms[0];
    ctx->stats.keccak_level_wide_us = us[1];
    ctx->stats.keccak_level_wide_perms = perms[1];
    ctx->stats.keccak_level_small_us = us[2];
    ctx->stats.keccak_level_small_perms = perms[2];
    ctx->stats.small_domain_us = us[3];
    ctx->stats.structure_us = us[4];
    ctx->stats.list_hash_us = us[5];
    ctx->stats.top_us = us[6];
    ctx->stats.top_perms = perms[6];
    ctx->stats.run_aware_us = us[4] + us[5];
    ctx->kev_n = 0;
    return ZIGZ_OK;
}

// what a build leaves in the context's stats at once (the counters' share follows in zigz_commit_roots)
static void publish_build_stats(zigz_ctx *ctx, const BuildResult &built) {
    ctx->stats.small_domain_columns = built.sd_cols;
    ctx->stats.run_aware_columns = built.run_cols;
    ctx->stats.run_aware_dense_nodes = built.run_dense;
    ctx->stats.cons_columns = ctx->stats.cons_dense_nodes = ctx->stats.cons_probe_distinct = 0;
}

struct zigz_merkle {
    uint32_t *d_vals;  // stored values (SimpleMerkleTree.values, merkle_tree.zig:291)
    uint8_t *d_tree;
    size_t n_values, npad;
    unsigned height;
};

extern "C" void zigz_merkle_destroy(zigz_ctx *ctx, zigz_merkle *t) {
    ZIGZ_ENTER(ctx);
    if (!t) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    if (t->d_vals) (void)hipFree(t->d_vals);
    if (t->d_tree) (void)hipFree(t->d_tree);
    delete t;
}

extern "C" zigz_status zigz_merkle_commit(zigz_ctx *ctx, const uint64_t *values, size_t n, uint8_t root[32],
                                          size_t *height, zigz_merkle **out) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (n == 0) return ZIGZ_ERR_EMPTY_VALUES;                      // merkle_tree.zig:284
    if (n > ((size_t)1 << 40)) return ZIGZ_ERR_TOO_MANY_VALUES;    // merkle_tree.zig:287 (device-size cap)
    if (!values || !root) return ZIGZ_ERR_INVALID_ARGUMENT;
    const size_t npad = ceil_pow2(n);
    zigz_merkle *t = new (std::nothrow) zigz_merkle();
    if (!t) return ZIGZ_ERR_OUT_OF_MEMORY;
    memset(t, 0, sizeof(*t));
    t->n_values = n;
    t->npad = npad;
    t->height = log2_floor(npad);
    zigz_status st = ZIGZ_OK;
    auto body = [&]() -> zigz_status {
        HIPCHK(ctx, hipMalloc((void **)&t->d_vals, n * 4));
        HIPCHK(ctx, hipMalloc((void **)&t->d_tree, tree_nodes(npad) * 32));
        CHK(upload_u64(ctx, values, n, t->d_vals, false));
        BuildResult built;
        const zigz_status bs = build_trees(ctx, t->d_vals, n, n, npad, t->d_tree, 1, false,
                                           BuildHints{ctx->small_domain_mask, ctx->run_aware_mask, ctx->cons_group_mask, ctx->run_aware_materialize, false}, &built);
        publish_build_stats(ctx, built);
        CHK(bs);
        void *d_root;  // the root leaves the device through the gather kernel: tree form -> canonical SHA3 bytes
        CHK(ws_get(ctx, WS_MISC, 64, &d_root));
        launch_gather_nodes(t->d_tree, tree_nodes(npad), tree_level_offset(npad, t->height), (uint8_t *)d_root, 1, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_root, 32, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(root, ctx->h_pin, 32);
        return ZIGZ_OK;
    };
    st = body();
    if (st != ZIGZ_OK) {
        zigz_merkle_destroy(ctx, t);
        return st;
    }
    if (height) *height = t->height;
    if (out) *out = t;
    else zigz_merkle_destroy(ctx, t);
    return ZIGZ_OK;
}

static zigz_status open_paths(zigz_ctx *ctx, const TreeRef &tree, unsigned height, const uint32_t *d_vals,
                              size_t val_stride, const uint64_t *h_idx, size_t ncols, uint8_t *siblings, uint8_t *dirs,
                              uint64_t *leaves) {
    ZIGZ_NOTHROW_BEGIN
    // device scratch layout: idx[ncols] u64 | sib[ncols*h*32] | leaf[ncols] u32 | dirs[ncols*h]
    const size_t sib_b = ncols * height * 32, idx_b = ncols * 8, leaf_b = ncols * 4, dir_b = ncols * height;
    void *w;
    CHK(ws_get(ctx, WS_OUT32, idx_b + sib_b + leaf_b + dir_b + 64, &w));
    uint8_t *base = (uint8_t *)w;
    uint64_t *d_idx = (uint64_t *)base;
    uint8_t *d_sib = base + idx_b;
    uint32_t *d_leaf = (uint32_t *)(d_sib + sib_b);
    uint8_t *d_dirs = (uint8_t *)(d_leaf + ncols);
    HIPCHK(ctx, hipMemcpyAsync(d_idx, h_idx, idx_b, hipMemcpyHostToDevice, ctx->stream));
    // (n_values = npad: leaf digests are virtual only in commit jobs, whose columns have exactly npad values)
    launch_paths(tree, tree.npad, height, d_vals, val_stride, d_idx, d_sib, d_dirs, d_leaf, ncols, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    std::vector<uint32_t> hl(ncols);
    if (sib_b) HIPCHK(ctx, hipMemcpyAsync(siblings, d_sib, sib_b, hipMemcpyDeviceToHost, ctx->stream));
    if (dir_b) HIPCHK(ctx, hipMemcpyAsync(dirs, d_dirs, dir_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hl.data(), d_leaf, leaf_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < ncols; c++) leaves[c] = hl[c];
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

extern "C" zigz_status zigz_merkle_open(zigz_ctx *ctx, const zigz_merkle *t, size_t index, uint8_t *siblings,
                                        uint8_t *dirs, uint64_t *leaf_value) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !t || !leaf_value) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (index >= t->n_values) return ZIGZ_ERR_INDEX_OUT_OF_BOUNDS;  // merkle_tree.zig:325 (values.len)
    if (t->height && (!siblings || !dirs)) return ZIGZ_ERR_INVALID_ARGUMENT;
    uint64_t idx = index;
    return open_paths(ctx, slab_tree_ref(t->d_tree, t->npad), t->height, t->d_vals, t->n_values, &idx, 1, siblings, dirs, leaf_value);
}

extern "C" zigz_status zigz_commit_open(zigz_ctx *ctx, const uint64_t *evals, size_t n, const zigz_merkle *tree,
                                        const uint64_t *point, size_t point_len, uint64_t *value, uint64_t *index,
                                        uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_value) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !tree || !value || !index || !leaf_value) return ZIGZ_ERR_INVALID_ARGUMENT;
    CHK(mle_check(n));
    if (point_len != log2_floor(n)) return ZIGZ_ERR_POINT_DIMENSION_MISMATCH;  // polynomial_commit.zig:92-94
    const uint32_t *d_ev = tree->d_vals;
    if (evals) {
        uint32_t *d;
        CHK(stage_in(ctx, evals, n, &d));
        d_ev = d;
    } else if (tree->n_values != n) {
        return ZIGZ_ERR_INVALID_ARGUMENT;
    }
    CHK(zigz_dev_mle_eval(ctx, d_ev, n, point, point_len, value));  // polynomial_commit.zig:97
    size_t idx = point_len == 0 ? 0 : (size_t)(point[0] % ((uint64_t)1 << point_len));  // pointToIndex, :178-183
    *index = idx;
    return zigz_merkle_open(ctx, tree, idx, siblings, dirs, leaf_value);  // :105
}

// ------------------------------------------------------------------ batched commit job (generateCommitments)
struct zigz_commit_job {
    zigz_ctx *ctx;
    size_t ncols, nv, N, col_stride;
    const uint32_t *d_cols;
    int state;  // 0 begun, 1 roots read, 2 opened
    hipEvent_t built;
    uint64_t const_cols; // hinted columns the structure pass found constant (summary word 7): not read by the eval
    uint64_t roots_seq;  // the DoneFlag sequence number of the (last) build's summary launch
    TreeRef tree;  // where the digests are (the context's WS_TREE / WS_RUNMETA / WS_CONSMETA workspaces)
    bool whole;    // built with every digest in node-addressed slabs (option run_aware_materialize)
    // the hints the job was begun with (a repeated build -- zigz_commit_roots, when a list ran out of room -- uses the same) and
    // what its build asked for (turned into stats when the counters have arrived; other calls may run in between)
    uint64_t m_small, m_run, m_cons;
    bool m_whole;
    cp::JobFacts facts;
    // a batched job (zigz_commit_begin_batch): nz proofs of ncols1 columns each; ncols = nz * ncols1.  arena: every proof's
    // build lives in its own zstride bytes of the context's WS_BATCH workspace (TreeRef::zstride); flat (nz > 1, zstride == 0):
    // the proofs' columns were gathered into one table of ncols columns and built densely like any other.
    unsigned nz;
    size_t ncols1, zstride;
    size_t off_r_ctr;  // byte offset of a proof's R list counters in its arena
    bool no_eval_skip;  // built without its structure passes (option debug_skip 2, measurement only): the "column changed" words
                        // were never written, so the eval must not take them for "constant"
};

// enqueues the builds of a job, the gather of its roots + counters into ONE pinned buffer, and the "built" event
static zigz_status job_build(zigz_commit_job *job) {
    zigz_ctx *ctx = job->ctx;
    const size_t ncols = job->ncols, nv = job->nv;
    CHK(timed_begin(ctx, 2));
    job->whole = job->m_whole;
    // (the hints of the job's begin, whatever the context's options say by now)
    BuildResult built;
    const zigz_status bs = build_trees(ctx, job->d_cols, job->col_stride, job->N, job->N, nullptr, ncols, ctx->timing,
                                       BuildHints{job->m_small, job->m_run, job->m_cons, job->m_whole, true}, &built);
    publish_build_stats(ctx, built);
    CHK(bs);
    job->tree = built.tree;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    // roots + the counters of the build -> contiguous device buffer -> pinned staging (async), then the "built" event
    // zero-copy: the summary kernel stores the roots and counters into the pinned host buffer itself (no copy command)
    const DoneFlag done = done_flag(ctx, 0);
    job->roots_seq = done.seq;
    launch_job_summary(job->tree, (unsigned)nv, ctx->h_roots, ncols,
                       built.run_cols ? ctx->d_run_count : nullptr, (built.sd_cols || built.cons_sd) ? ctx->d_sd_fallbacks : nullptr,
                       built.cons_hinted ? ctx->d_cons_count : nullptr, ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(job->built, ctx->stream));
    // hinted columns take levels 0 and 1 (N + N/2 digests) from the tables (waves that had to hash are counted in
    // small_domain_fallback_waves, read in zigz_commit_roots; they are not added back here)
    job->facts = cp::JobFacts{built.run_cols, built.run_dense, built.sd_cols, built.cons_hinted, built.cons_levels_nodes, built.cons_sd,
                              (uint64_t)ncols * (2 * job->N - 1) - built.sd_cols * (job->N + job->N / 2), job->N};
    job->no_eval_skip = ctx->debug_skip == 2;
    return ZIGZ_OK;
}

// A new job of nz proofs (0: a single job) of ncols1 columns and 2^nv rows each becomes the context's active job once
// build(job) has queued its build.
template <class Build>
static zigz_status job_new(zigz_ctx *ctx, unsigned nz, size_t ncols1, size_t nv, zigz_commit_job **out, Build build) {
    if (ctx->active_job) {
        set_err(ctx, "a commit job is already active on this context");
        return ZIGZ_ERR_BAD_STATE;
    }
    zigz_commit_job *job = new (std::nothrow) zigz_commit_job();
    if (!job) return ZIGZ_ERR_OUT_OF_MEMORY;
    memset(job, 0, sizeof(*job));
    job->ctx = ctx;
    job->nz = nz;
    job->ncols1 = nz ? ncols1 : 0;
    job->ncols = ncols1 * (nz ? nz : 1);
    job->nv = nv;
    job->N = (size_t)1 << nv;
    auto body = [&]() -> zigz_status {
        HIPCHK(ctx, hipEventCreateWithFlags(&job->built, hipEventDisableTiming));
        return build(job);
    };
    const zigz_status st = body();
    if (st != ZIGZ_OK) {
        if (job->built) (void)hipEventDestroy(job->built);
        delete job;
        return st;
    }
    ctx->active_job = job;
    *out = job;
    return ZIGZ_OK;
}

static zigz_status job_begin(zigz_ctx *ctx, const uint32_t *d_cols, size_t ncols, size_t col_stride, size_t nv,
                             zigz_commit_job **out) {
    return job_new(ctx, 0, ncols, nv, out, [&](zigz_commit_job *job) {
        job->col_stride = col_stride;
        job->d_cols = d_cols;
        job->m_small = ctx->small_domain_mask;
        job->m_run = ctx->run_aware_mask;
        job->m_cons = ctx->cons_group_mask;
        job->m_whole = ctx->run_aware_materialize;
        return job_build(job);
    });
}

// ---- a batched job: several proofs' columns in ONE commit job (zigz_commit_begin_batch)
// Small traces make a proof's ~35 launches mostly latency (2^16: 13 us of work per launch); nz proofs of the same shape share
// every launch instead.  Two forms, chosen by the size:
//   flat  (N < 2^15: trees that are built densely anyway) -- the proofs' columns are gathered into one table of nz * ncols1
//         columns and committed like any other table;
//   arena (2^15 <= N <= 2^18: the structure-aware levels) -- every proof gets an arena with the same layout for everything
//         its build reads or writes (a copy of its columns, list counters, lists, leader tables, content-addressing table,
//         digest stores, upper levels, slabs for a dropped group), the kernels take the proof from gridDim.z and move every
//         pointer by proof * arena size (kernels.hpp: TreeRef::zstride).  The lists get their WORST-CASE room (every node
//         hashed: affordable at these sizes, ~0.25 GiB per proof at 2^16), so a batched build is never repeated; every column
//         must be hinted run-aware or member of the content-addressed group (the witness's 43 are: host/prover.cpp).
static zigz_status job_build_batch_arena(zigz_commit_job *job, const uint32_t *const *srcs, size_t src_stride) {
    zigz_ctx *ctx = job->ctx;
    const size_t nc = job->ncols1, N = job->N, npad = N;
    const unsigned nz = job->nz, height = (unsigned)job->nv;
    ColMap R{}, G{};
    for (size_t c = 0; c < nc; c++) {
        if ((job->m_cons >> c) & 1) G.c[G.n++] = (uint8_t)c;
        else if ((job->m_run >> c) & 1) R.c[R.n++] = (uint8_t)c;
        else return ZIGZ_ERR_INVALID_ARGUMENT;  // (a densely built column: not in this form)
    }
    const size_t stride = N;  // column stride inside an arena
    TreeRef t = empty_tree_ref(npad);
    const cp::Shape shape = tree_ref_lists(t, R, G, nc, nullptr, nullptr);
    for (unsigned k = 0; k < G.n; k++) t.slab_of_col[G.c[k]] = (signed char)k;  // where a dropped group's columns are built densely
    // ---- the arena's layout (byte offsets, the same for every proof): columns | R counters | G counters | the lists' storage
    // (cp::plan_arena) | the group's slabs
    const size_t o_cols = 0, o_rctr = align256(nc * stride * 4), o_gctr = o_rctr + align256(RUN_CTR_WORDS * 8);
    const cp::Plan plan = cp::plan_arena(shape, o_gctr + align256(RUN_CTR_WORDS * 8));
    const size_t o_slab = plan.total[0], o_keys = plan.off[cp::G_KEYS], key_bytes = plan.bytes[cp::G_KEYS];
    const size_t S = o_slab + align256((size_t)G.n * tree_nodes(npad) * 32);
    if ((size_t)nz * S > ((size_t)48 << 30)) return ZIGZ_ERR_OUT_OF_MEMORY;
    void *w;
    const void *w_before = ctx->ws[WS_BATCH];
    const size_t n_res = nz > ctx->batch_reserve ? nz : ctx->batch_reserve;
    if ((size_t)n_res * S <= ((size_t)48 << 30)) CHK(ws_get(ctx, WS_BATCH, (size_t)n_res * S, &w));
    else CHK(ws_get(ctx, WS_BATCH, (size_t)nz * S, &w));
    uint8_t *a0 = (uint8_t *)w;
    // the content-addressing tables (generation-tagged slots): cleared when the workspace or the layout is new, or the
    // generations run out -- all nz of them with one strided fill
    // (generations of their own -- batch_gen --: the single jobs' table in WS_CONS starts its count over whenever IT is new)
    if (G.n && (w != w_before || ctx->batch_tab_S != S || ctx->batch_tab_nz < nz || ctx->batch_tab_off != o_keys ||
                ctx->batch_gen == 0 || ctx->batch_gen + RUN_MAX_LEVELS + 1 >= 4096)) {
        const size_t n_tabs = ctx->ws_bytes[WS_BATCH] / S;  // (every arena the workspace has room for: a later, larger batch finds them clear)
        HIPCHK(ctx, hipMemset2DAsync(a0 + o_keys, S, 0, key_bytes, n_tabs, ctx->stream));
        ctx->batch_tab_S = S;
        ctx->batch_tab_nz = (unsigned)n_tabs;
        ctx->batch_tab_off = o_keys;
        ctx->batch_gen = 1;
    }
    MerkleBuild b{};
    b.vals = (const uint32_t *)(a0 + o_cols);
    b.val_stride = stride;
    b.n_values = N;
    b.npad = npad;
    b.rcols = R;
    b.gcols = G;
    uint8_t *const base[cp::N_SPACES] = {a0};
    point_at_regions(b, t, plan, base, (unsigned long long *)(a0 + o_gctr));
    if (R.n) b.r_ctr = (unsigned long long *)(a0 + o_rctr);
    if (G.n) {
        t.slab = a0 + o_slab;
        b.g_has_slabs = 1;
        b.g_gen = ctx->batch_gen;
        ctx->batch_gen += t.top + 1;
    }
    b.t = t;
    set_zstride(b, S, nz);
    t = b.t;
    ColSrcs cs{};
    for (unsigned z = 0; z < nz; z++) cs.p[z] = srcs[z];
    launch_gather_cols(cs, nz, nc, N, src_stride, (uint32_t *)(a0 + o_cols), stride, S, ctx->stream);
    launch_zero_counters(nullptr, R.n ? b.r_ctr : nullptr, G.n ? b.g_ctr : nullptr, ctx->stream, nz, S);
    if (ctx->debug_skip != 2) launch_structure(b, ctx->stream, ctx->debug_skip == 0);
    for (unsigned l = 0; l <= t.top; l++)
        if (ctx->debug_skip != 1) launch_level_hash(b, l, ctx->stream, nullptr, 0, ctx->debug_skip == 0);
    if (height && ctx->debug_skip != 1) launch_merkle_top(t, t.top, height, nc, ctx->stream, nullptr);
    HIPCHK(ctx, hipGetLastError());
    job->tree = t;
    job->d_cols = (const uint32_t *)(a0 + o_cols);
    job->col_stride = stride;
    job->zstride = S;
    job->off_r_ctr = o_rctr;
    job->whole = false;
    const DoneFlag done = done_flag(ctx, 0);
    job->roots_seq = done.seq;
    launch_job_summary(t, height, ctx->h_roots, nc, R.n ? b.r_ctr : nullptr, nullptr, G.n ? b.g_ctr : nullptr, ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(job->built, ctx->stream));
    const uint64_t level_nodes = list_level_nodes(npad);
    job->facts = cp::JobFacts{R.n, (uint64_t)R.n * level_nodes, 0, G.n, level_nodes, 0, (uint64_t)nc * (2 * N - 1), N};
    job->no_eval_skip = ctx->debug_skip == 2;
    return ZIGZ_OK;
}

extern "C" zigz_status zigz_commit_begin_batch(zigz_ctx *ctx, const uint32_t *const *d_cols, size_t nproofs, size_t ncols,
                                               size_t col_stride, size_t nv, zigz_commit_job **out) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !d_cols || !out || ncols == 0 || nproofs == 0 || nproofs > BATCH_MAX || nv > 40) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (ncols * nproofs > ROOTS_MAX_COLS || col_stride < ((size_t)1 << nv)) return ZIGZ_ERR_INVALID_ARGUMENT;
    for (size_t z = 0; z < nproofs; z++)
        if (!d_cols[z]) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (nproofs == 1) return job_begin(ctx, d_cols[0], ncols, col_stride, nv, out);
    const size_t N = (size_t)1 << nv;
    const bool arena = N >= RUN_MIN_LEAVES && N <= ((size_t)1 << BATCH_ARENA_MAX_NV) && ncols <= 64 && (ctx->run_aware_mask || ctx->cons_group_mask);
    return job_new(ctx, (unsigned)nproofs, ncols, nv, out, [&](zigz_commit_job *job) -> zigz_status {
        if (N >= RUN_MIN_LEAVES && !arena) return ZIGZ_ERR_INVALID_ARGUMENT;  // (large tables: one job per proof)
        if (arena) {
            job->m_small = 0;
            job->m_run = ctx->run_aware_mask;
            job->m_cons = ctx->cons_group_mask;
            return job_build_batch_arena(job, d_cols, col_stride);
        }
        // flat: one table of nz * ncols columns, built densely (no hints: they are per 64 columns of ONE proof)
        const size_t dstride = N < 4 ? 4 : N;
        void *d;
        CHK(ws_get(ctx, WS_COLS, (job->nz > ctx->batch_reserve ? job->nz : ctx->batch_reserve) * ncols * dstride * 4, &d));
        ColSrcs cs{};
        for (size_t z = 0; z < nproofs; z++) cs.p[z] = d_cols[z];
        launch_gather_cols(cs, job->nz, ncols, N, col_stride, (uint32_t *)d, dstride, ncols * dstride * 4, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
        job->d_cols = (const uint32_t *)d;
        job->col_stride = dstride;
        job->m_small = job->m_run = job->m_cons = 0;
        job->m_whole = false;
        return job_build(job);
    });
}

extern "C" zigz_status zigz_commit_begin_dev(zigz_ctx *ctx, const uint32_t *d_cols, size_t ncols, size_t col_stride,
                                             size_t nv, zigz_commit_job **out) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !d_cols || !out || ncols == 0 || nv > 40) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (ncols > ROOTS_MAX_COLS) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (col_stride < ((size_t)1 << nv)) return ZIGZ_ERR_INVALID_ARGUMENT;
    return job_begin(ctx, d_cols, ncols, col_stride, nv, out);
}

extern "C" zigz_status zigz_commit_begin(zigz_ctx *ctx, const uint64_t *cols, size_t ncols, size_t col_stride,
                                         size_t nv, zigz_commit_job **out) {
    ZIGZ_ENTER(ctx);
    if (!ctx || !cols || !out || ncols == 0 || nv > 40) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (ncols > ROOTS_MAX_COLS) return ZIGZ_ERR_INVALID_ARGUMENT;
    const size_t N = (size_t)1 << nv;
    if (col_stride < N) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (ctx->active_job) return ZIGZ_ERR_BAD_STATE;
    const size_t dstride = N < 4 ? 4 : N;
    void *d;
    CHK(ws_get(ctx, WS_COLS, ncols * dstride * 4, &d));
    uint32_t *d_cols = (uint32_t *)d;
    if (col_stride == N && dstride == N) {
        CHK(upload_u64(ctx, cols, ncols * N, d_cols, false));
    } else {
        for (size_t c = 0; c < ncols; c++) CHK(upload_u64(ctx, cols + c * col_stride, N, d_cols + c * dstride, false));
    }
    return job_begin(ctx, d_cols, ncols, dstride, nv, out);
}

extern "C" zigz_status zigz_commit_roots(zigz_commit_job *job, uint8_t *roots) {
    if (job) ZIGZ_ENTER(job->ctx);
    if (!job || !roots) return ZIGZ_ERR_INVALID_ARGUMENT;
    zigz_ctx *ctx = job->ctx;
    if (job->state != 0) return ZIGZ_ERR_BAD_STATE;
    const unsigned long long *h_cnt = (const unsigned long long *)(ctx->h_roots + job->ncols * 32);
    for (int attempt = 0;; attempt++) {
        const unsigned long long *h_done = (const unsigned long long *)(ctx->h_roots + ROOTS_MAX_COLS * 32 + JOB_SUMMARY_WORDS * 8);
        if (!(g_sleep_wait.load() && !ctx->timing && sleep_wait(h_done, job->roots_seq)))
            HIPCHK(ctx, hipEventSynchronize(job->built));
        // What the lists of the structure-aware levels needed: the context remembers it for its next builds, and a build that
        // ran out of room (or found its group dropped with nowhere to build the columns densely) is repeated here with more.
        // This is the one place where a proof may pay for a second build: the first time a context meets a new kind of trace.
        bool again = false;
        if (job->zstride) {  // a batched job's lists have their worst-case room: nothing to learn, nothing can have run out
            for (unsigned z = 0; z < job->nz; z++)
                if (h_cnt[(size_t)z * JOB_SUMMARY_WORDS + cp::SUM_FLAGS]) {
                    set_err(ctx, "batched commit job: a list ran out of its worst-case room (proof %u)", z);
                    return ZIGZ_ERR_BAD_STATE;
                }
        } else if (job->tree.lists) {
            again = cp::learn_caps(ctx->caps, h_cnt, job->facts);
        }
        if (!again) break;
        if (attempt >= 3) {
            set_err(ctx, "commit job: the lists of the structure-aware levels still do not fit after %d builds", attempt + 1);
            return ZIGZ_ERR_BAD_STATE;
        }
        ctx->stats.rebuilds++;
        CHK(job_build(job));
    }
    memcpy(roots, ctx->h_roots, job->ncols * 32);
    // the stats: the sums over the job's proofs (a flat batch is ONE build of all its columns)
    job->const_cols = cp::job_stats(ctx->stats, h_cnt, job->zstride ? job->nz : 1, job->facts);
    if (ctx->timing && !job->zstride) {
        float ms = 0;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
        ctx->stats.merkle_build_us = (double)ms * 1000.0;
        CHK(keccak_times_collect(ctx));
    }
    job->state = 1;
    return ZIGZ_OK;
}

extern "C" zigz_status zigz_commit_open_all(zigz_commit_job *job, const uint64_t *points, uint64_t *values,
                                            uint64_t *indices, uint64_t *leaves, uint8_t *siblings, uint8_t *dirs) {
    ZIGZ_NOTHROW_BEGIN
    if (job) ZIGZ_ENTER(job->ctx);
    if (!job || !values || !indices || !leaves) return ZIGZ_ERR_INVALID_ARGUMENT;
    zigz_ctx *ctx = job->ctx;
    if (job->state != 1) return ZIGZ_ERR_BAD_STATE;
    const size_t nv = job->nv, ncols = job->ncols;
    if (nv && (!points || !siblings || !dirs)) return ZIGZ_ERR_INVALID_ARGUMENT;
    // What a proof needs back -- 43 evaluations, leaves, sibling digests, directions: ~30 KB -- is written by the kernels
    // straight into the pinned staging buffer, and the indices are read from it: no copy command at all, one wait (0.51 vs
    // 0.52 ms of GPU per proof with 14 lanes; ONE packed copy through the same buffer was slower than the five small copies
    // to pageable memory of the fallback below: 0.56 ms).
    const size_t sib_b = ncols * nv * 32, leaf_b = ncols * 4, val_b = ncols * 4, dir_b = ncols * nv;
    const size_t out_b = sib_b + leaf_b + val_b + dir_b;
    if (out_b <= PIN_WORDS * 8 / 2 && nv * ncols * 4 + ncols * 8 <= PIN_WORDS * 8 / 2) {
        uint8_t *h = (uint8_t *)ctx->h_pin;
        uint8_t *z_sib = h;
        uint32_t *z_leaf = (uint32_t *)(h + sib_b), *z_val = z_leaf + ncols;
        uint8_t *z_dirs = (uint8_t *)(z_val + ncols);
        uint64_t *h_idx = ctx->h_pin + PIN_WORDS - ncols;
        for (size_t c = 0; c < ncols; c++) {
            h_idx[c] = nv == 0 ? 0 : points[c * nv] % ((uint64_t)1 << nv);  // pointToIndex
            indices[c] = h_idx[c];
        }
        // columns the run-aware structure pass of THIS job found constant are not read again (EvalSkip, kernels.hpp): of the 43
        // witness columns of a program that uses a handful of registers, most.  A batched job in arenas: column c = column
        // c % ncols1 of proof c / ncols1, always in the radix form.
        const bool arena = job->zstride != 0;
        const bool use = job->facts.run_cols && !job->no_eval_skip && (arena || (job->tree.lists && job->col_stride >= job->N));
        EvalSkip skip;
        if (arena) {
            skip.ncols1 = (unsigned)job->ncols1;
            skip.z_in = job->zstride / 4;
            skip.z_changed = job->zstride / 8;
        }
        if (arena || use) memcpy(skip.y_of_col, job->tree.y_of_col, sizeof(skip.y_of_col));
        // (the job's own counters: no other build on the context adds to them)
        const unsigned long long *r_ctr = arena ? (const unsigned long long *)((const uint8_t *)ctx->ws[WS_BATCH] + job->off_r_ctr) : ctx->d_run_count;
        if (use) skip.changed = r_ctr + RUN_CHANGED;
        const size_t n_const = use ? job->const_cols : 0;
        if (arena || use) ctx->stats.eval_constant_columns = n_const;
        CHK(timed_begin(ctx, 4));
        EvalFinish fin;  // (the radix form leaves the values to the paths launch: one evaluation launch instead of four)
        if (arena) CHK(dev_eval_radix(ctx, job->d_cols, job->col_stride, ncols, nv, points, z_val, &skip, n_const, &fin));
        else CHK(dev_eval_folds(ctx, job->d_cols, job->col_stride, ncols, nv, points, z_val, use ? &skip : nullptr, n_const, &fin));
        CHK(timed_end(ctx, 4, &ctx->stats.eval_us));
        const DoneFlag done = done_flag(ctx, 1);
        launch_paths(job->tree, job->tree.npad, (unsigned)nv, job->d_cols, job->col_stride, h_idx, z_sib, z_dirs, z_leaf,
                     job->zstride ? job->ncols1 : ncols, ctx->stream, done, &fin);
        HIPCHK(ctx, hipGetLastError());
        if (!(g_sleep_wait.load() && !ctx->timing && sleep_wait(done.flag, done.seq)))
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (sib_b) memcpy(siblings, z_sib, sib_b);
        for (size_t c = 0; c < ncols; c++) {
            leaves[c] = z_leaf[c];
            values[c] = z_val[c];
        }
        if (dir_b) memcpy(dirs, z_dirs, dir_b);
        CHK(bind_pool_collect(ctx));
        job->state = 2;
        return ZIGZ_OK;
    }
    if (job->zstride) {
        set_err(ctx, "batched commit job: the openings do not fit the staging buffer");
        return ZIGZ_ERR_INVALID_ARGUMENT;
    }
    void *dv;
    CHK(ws_get(ctx, WS_SCRATCH, ncols * 4 + 64, &dv));
    CHK(timed_begin(ctx, 4));
    CHK(dev_eval_folds(ctx, job->d_cols, job->col_stride, ncols, nv, points, (uint32_t *)dv));
    CHK(timed_end(ctx, 4, &ctx->stats.eval_us));
    std::vector<uint32_t> hv(ncols);
    HIPCHK(ctx, hipMemcpyAsync(hv.data(), dv, ncols * 4, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint64_t> idx(ncols);
    for (size_t c = 0; c < ncols; c++) {
        idx[c] = nv == 0 ? 0 : points[c * nv] % ((uint64_t)1 << nv);  // pointToIndex
        indices[c] = idx[c];
    }
    CHK(open_paths(ctx, job->tree, (unsigned)nv, job->d_cols, job->col_stride, idx.data(), ncols, siblings, dirs, leaves));
    for (size_t c = 0; c < ncols; c++) values[c] = hv[c];
    CHK(bind_pool_collect(ctx));
    job->state = 2;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(job->ctx)
}

// k openings of the job's trees in shared launches (kernels.hip: k_open_many), chunked through pinned memory like
// zigz_merkle_open_many.  A batched job in arenas runs proof z's openings in grid plane z (TreeRef's pointers follow
// blockIdx.z), so a chunk's descriptors are sorted by proof; each carries its opening's position in the chunk.
extern "C" zigz_status zigz_commit_open_many(zigz_commit_job *job, size_t k, const uint32_t *cols, const uint64_t *indices,
                                             uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values, size_t *bad_index) {
    if (job) ZIGZ_ENTER(job->ctx);
    if (!job) return ZIGZ_ERR_INVALID_ARGUMENT;
    zigz_ctx *ctx = job->ctx;
    if (job->state != 1 && job->state != 2) return ZIGZ_ERR_BAD_STATE;
    if (k == 0) return ZIGZ_OK;
    size_t bad = 0;
    switch (mo::check_openings(k, cols, indices, job->ncols, nullptr, job->N, &bad)) {
    case mo::OK: break;
    case mo::BAD_ARGUMENT: return ZIGZ_ERR_INVALID_ARGUMENT;
    case mo::BAD_TREE:
        set_err(ctx, "opening %zu names column %u of a job of %zu", bad, cols[bad], job->ncols);
        return fail_at(bad_index, bad, ZIGZ_ERR_INVALID_ARGUMENT);
    case mo::BAD_INDEX: return fail_at(bad_index, bad, ZIGZ_ERR_INDEX_OUT_OF_BOUNDS);
    }
    const size_t nv = job->nv;
    if (!leaf_values || (nv && (!siblings || !dirs))) return ZIGZ_ERR_INVALID_ARGUMENT;
    ZIGZ_NOTHROW_BEGIN
    std::vector<uint64_t> off(k + 1);
    for (size_t j = 0; j <= k; j++) off[j] = j * nv;
    const std::vector<mo::Chunk> chunks = mo::plan_chunks(off, k, OPEN_CHUNK_BYTES, false);
    const unsigned nz = job->zstride ? job->nz : 1;
    const size_t ncols1 = job->zstride ? job->ncols1 : job->ncols;
    size_t most = 0, most_n = 0;
    for (const mo::Chunk &c : chunks) {
        most = std::max(most, c.bytes);
        most_n = std::max(most_n, c.hi - c.lo);
    }
    uint8_t *pin;
    CHK(pinned(ctx, (chunks.size() > 1 ? 2 : 1) * most, &pin));
    void *ws;
    CHK(ws_get(ctx, WS_OPEN, most_n * sizeof(mo::Desc), &ws));
    auto launch = [&](size_t ci, DoneFlag *done) -> zigz_status {
        const mo::Chunk &c = chunks[ci];
        uint8_t *st = pin + (ci & 1) * most;
        const size_t n = c.hi - c.lo;
        OpenManyZ zf{};  // counting sort by proof: first[z + 1] counts, then starts
        for (size_t j = c.lo; j < c.hi; j++) zf.first[cols[j] / ncols1 + 1]++;
        for (unsigned z = 0; z < nz; z++) zf.first[z + 1] += zf.first[z];
        uint32_t next[BATCH_MAX];
        memcpy(next, zf.first, sizeof(next));
        mo::Desc *hd = (mo::Desc *)st;
        for (size_t j = c.lo; j < c.hi; j++)
            hd[next[cols[j] / ncols1]++] = mo::Desc{indices[j], (uint32_t)(cols[j] % ncols1), (uint32_t)(j - c.lo)};
        // (the previous chunk's launch reads the descriptors: the copy queues behind it on the stream)
        HIPCHK(ctx, hipMemcpyAsync(ws, st, n * sizeof(mo::Desc), hipMemcpyHostToDevice, ctx->stream));
        *done = done_flag(ctx, 3 + (int)(ci & 1));
        launch_open_many(job->tree, (unsigned)nv, job->d_cols, job->col_stride, (const mo::Desc *)ws, zf, nz, st + c.off_sib,
                         st + c.off_dirs, (uint64_t *)(st + c.off_leaf), ctx->stream, *done);
        HIPCHK(ctx, hipGetLastError());
        return ZIGZ_OK;
    };
    auto take = [&](size_t ci) {
        const mo::Chunk &c = chunks[ci];
        const uint8_t *st = pin + (ci & 1) * most;
        if (c.slots) {
            memcpy(siblings + 32 * c.slot0, st + c.off_sib, 32 * c.slots);
            memcpy(dirs + c.slot0, st + c.off_dirs, c.slots);
        }
        memcpy(leaf_values + c.lo, st + c.off_leaf, 8 * (c.hi - c.lo));
    };
    return run_open_chunks(ctx, chunks.size(), launch, take);
    ZIGZ_NOTHROW_END(ctx)
}

extern "C" zigz_status zigz_commit_job_tree(zigz_commit_job *job, const void **d_tree, size_t *bytes_per_column) {
    if (job) ZIGZ_ENTER(job->ctx);
    if (!job || !d_tree || !bytes_per_column) return ZIGZ_ERR_INVALID_ARGUMENT;
    // node-addressed trees of every column exist only when nothing was list-built, or the job was begun with
    // "run_aware_materialize" (otherwise the list-built levels live in list order: there is no whole tree to look at)
    if (job->tree.lists && !job->whole) return ZIGZ_ERR_BAD_STATE;
    HIPCHK(job->ctx, hipEventSynchronize(job->built));
    *d_tree = job->tree.slab;
    *bytes_per_column = tree_nodes(job->N) * 32;
    return ZIGZ_OK;
}

extern "C" void zigz_commit_end(zigz_commit_job *job) {
    if (job) ZIGZ_ENTER(job->ctx);
    if (!job) return;
    zigz_ctx *ctx = job->ctx;
    (void)hipStreamSynchronize(ctx->stream);
    if (job->built) (void)hipEventDestroy(job->built);
    if (ctx->active_job == job) ctx->active_job = nullptr;
    delete job;
}

