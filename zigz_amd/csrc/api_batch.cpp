// C ABI of libzigz_hip.so, part 5: the batched provers -- k independent sumchecks (and Lasso proofs) in shared launches.
//
// Schedule (DESIGN.md "Batched provers"): every table keeps the single-table radix schedule (sumcheck_host.hpp: radix_run_batch
// next to radix_run) -- a table of n > HOST_TAIL_MAX elements runs a block-sums pass with k = min(log n - 8, 10), then
// folds until m <= 1024; a smaller one goes straight to the tail -- but each GPU pass serves EVERY table still in play in one
// launch (sumcheck_batch.hip), and between passes the host runs each table's k rounds on its own block sums with its own
// transcript (RadixProver).  Tables that finish early drop out of later passes; all remaining tables are read back in one
// hand-off.  Exact arithmetic throughout, so every table's rounds, point and final_eval are those of a call of its own.
#include "api_internal.hpp"

#include <algorithm>
#include <array>

using namespace zk;

namespace zk {
void flat_commit_batch(const uint32_t *const *ev, const size_t *n, size_t count, uint8_t (*out)[32]);  // host_sponge_batch.cpp
}

namespace {

// one instance of zigz_lasso_prove_batch (entry i of its arrays) and where its results go
struct LassoInst {
    const uint64_t *table;
    size_t table_rows;
    const uint64_t *queries;
    size_t n_queries, n_in, n_out;
    const uint64_t *mapping;
    size_t n_mapping;
};
struct LassoOut {
    uint64_t *rounds, *point;
};

// ------------------------------------------------------------------ the passes on the GPU
// Workspaces (sized from the batch's first pass, which is its largest, and kept by the context; no allocation inside the loop):
//   WS_SCBATCH   descriptors + weights (device mirror of the staging area) | stage sums | fold partials | two output regions
//   pinned       published sums / tails | staging (ctx->h_pin when the batch fits it, else ctx->h_batch)
struct GpuBatch {
    zigz_ctx *ctx;
    size_t k;
    std::vector<const uint32_t *> cur;
    std::vector<size_t> len, part_off, out_off;
    std::vector<unsigned> parity;
    // device
    uint8_t *d_stage;
    unsigned long long *d_sums, *d_part;
    uint32_t *d_out[2];
    // pinned
    uint8_t *h_out, *h_stage;
    size_t stage_bytes;
    size_t tail_desc_off, weights_off;  // inside the staging area
};

BatchPublish make_pub(const DoneFlag &done, void *h_dst, unsigned long long *d_sums, size_t n) {
    BatchPublish p;
    p.h_dst = h_dst;
    p.d_sums = d_sums;
    p.n = n;
    p.count = done.count;
    p.flag = done.flag;
    p.seq = done.seq;
    return p;
}

zigz_status gpu_batch_init(zigz_ctx *ctx, GpuBatch &g, size_t k, const uint32_t *const *d_tables, const size_t *ns) {
    g.ctx = ctx;
    g.k = k;
    g.cur.assign(d_tables, d_tables + k);
    g.len.assign(ns, ns + k);
    g.part_off.assign(k, 0);
    g.out_off.assign(k, 0);
    g.parity.assign(k, 0);
    size_t sums_w = 0, part_w = 0, out_w = 0, w_words = 0, tail_w = 0;
    for (size_t i = 0; i < k; i++) {
        if (const unsigned kk = radix_stage_k(ns[i])) {
            const size_t nb = (size_t)1 << kk, m0 = ns[i] >> kk, groups = radix_fold_groups(nb);
            g.part_off[i] = part_w;
            g.out_off[i] = out_w;
            sums_w += nb;
            w_words += nb;
            part_w += groups * m0;
            out_w += (m0 + 3) & ~(size_t)3;  // every output table 16-byte aligned
            tail_w += HOST_TAIL_MAX;
        } else {
            tail_w += ns[i];
        }
    }
    const size_t desc = align256(k * sizeof(BatchTab));
    g.weights_off = 2 * desc;
    g.tail_desc_off = g.weights_off + align256(w_words * 4);
    g.stage_bytes = g.tail_desc_off + desc;
    const size_t out_bytes = align256(std::max(sums_w * 8, tail_w * 4));
    // pinned: the context's buffer when the batch fits it
    uint8_t *pin;
    CHK(pinned(ctx, out_bytes + g.stage_bytes, &pin));
    g.h_out = pin;
    g.h_stage = pin + out_bytes;
    // device
    const size_t sums_bytes = align256(sums_w * 8 + 8), part_bytes = align256(part_w * 8 + 8), outs = align256(out_w * 4 + 16);
    void *ws;
    CHK(ws_get(ctx, WS_SCBATCH, g.stage_bytes + sums_bytes + part_bytes + 2 * outs, &ws));
    g.d_stage = (uint8_t *)ws;
    g.d_sums = (unsigned long long *)(g.d_stage + g.stage_bytes);
    g.d_part = (unsigned long long *)((uint8_t *)g.d_sums + sums_bytes);
    g.d_out[0] = (uint32_t *)((uint8_t *)g.d_part + part_bytes);
    g.d_out[1] = (uint32_t *)((uint8_t *)g.d_out[0] + outs);
    // the stage sums start at zero (one fill per batch; every publish leaves what it read zero)
    if (sums_w) HIPCHK(ctx, hipMemsetAsync(g.d_sums, 0, sums_w * 8, ctx->stream));
    return ZIGZ_OK;
}

// 16-byte chunks per lane of a block-sums wave: ~8192 waves over the whole pass (k_block_sums' rule), inside one block
unsigned bsums_iters(size_t total, size_t m) {
    size_t iters = (total / 256) / 8192;
    size_t p2 = 1;
    while (p2 * 2 <= iters) p2 *= 2;
    iters = p2;
    if (iters > m / 256) iters = m / 256;
    if (iters > 64) iters = 64;
    return (unsigned)(iters < 1 ? 1 : iters);
}

zigz_status gpu_batch_block_sums(void *user, size_t count, const size_t *tables, const unsigned *ks, uint64_t *sums) {
    GpuBatch *g = (GpuBatch *)user;
    zigz_ctx *ctx = g->ctx;
    BatchTab *d = (BatchTab *)g->h_stage;
    size_t total = 0, so = 0;
    for (size_t j = 0; j < count; j++) total += g->len[tables[j]];
    unsigned wg = 0;
    for (size_t j = 0; j < count; j++) {
        const size_t i = tables[j], n = g->len[i];
        BatchTab b{};
        b.in = g->cur[i];
        b.sums = g->d_sums + so;
        b.log2_n = log2_floor(n);
        b.k = ks[j];
        b.iters = bsums_iters(total, n >> ks[j]);
        b.first_wg = wg;
        d[j] = b;
        const size_t waves = n / (256 * (size_t)b.iters);
        wg += (unsigned)((waves + BATCH_WG / 64 - 1) / (BATCH_WG / 64));
        so += (size_t)1 << ks[j];
    }
    HIPCHK(ctx, hipMemcpyAsync(g->d_stage, d, count * sizeof(BatchTab), hipMemcpyHostToDevice, ctx->stream));
    const DoneFlag done = done_flag(ctx, 2);
    launch_batch_block_sums((const BatchTab *)g->d_stage, (unsigned)count, wg, ctx->stream);
    launch_batch_publish(make_pub(done, g->h_out, g->d_sums, so), ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    memcpy(sums, g->h_out, so * 8);
    return ZIGZ_OK;
}

zigz_status gpu_batch_fold(void *user, size_t count, const size_t *tables, const unsigned *ks, const uint64_t *weights,
                           const unsigned *knext, uint64_t *next_sums) {
    GpuBatch *g = (GpuBatch *)user;
    zigz_ctx *ctx = g->ctx;
    const size_t desc = align256(g->k * sizeof(BatchTab));
    BatchTab *fd = (BatchTab *)g->h_stage, *nd = (BatchTab *)(g->h_stage + desc);
    uint32_t *hw = (uint32_t *)(g->h_stage + g->weights_off);
    const uint32_t *dw = (const uint32_t *)(g->d_stage + g->weights_off);
    size_t wo = 0, so = 0;
    unsigned wg_f = 0, wg_n = 0;
    for (size_t j = 0; j < count; j++) {
        const size_t i = tables[j], n = g->len[i], nb = (size_t)1 << ks[j], m = n >> ks[j];
        for (size_t b = 0; b < nb; b++) hw[wo + b] = host_to_mont(weights[wo + b]);
        uint32_t *out = g->d_out[g->parity[i] & 1] + g->out_off[i];
        BatchTab f{};
        f.in = g->cur[i];
        f.part = g->d_part + g->part_off[i];
        f.w = dw + wo;
        f.log2_n = log2_floor(n);
        f.k = ks[j];
        f.first_wg = wg_f;
        fd[j] = f;
        wg_f += (unsigned)(((m / 4 + BATCH_WG - 1) / BATCH_WG) * radix_fold_groups(nb));
        BatchTab z = f;
        z.out = out;
        z.first_wg = wg_n;
        if (knext[j]) {
            z.sums = g->d_sums + so;
            z.log2_m2 = log2_floor(m) - knext[j];
            so += (size_t)1 << knext[j];
        }
        nd[j] = z;
        wg_n += (unsigned)((m + BATCH_WG - 1) / BATCH_WG);
        wo += nb;
    }
    // one copy: fold descriptors | finalize descriptors | weights
    HIPCHK(ctx, hipMemcpyAsync(g->d_stage, g->h_stage, g->weights_off + wo * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_batch_fold((const BatchTab *)g->d_stage, (unsigned)count, wg_f, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    DoneFlag done{};
    if (so) done = done_flag(ctx, 2);
    launch_batch_finalize((const BatchTab *)(g->d_stage + desc), (unsigned)count, wg_n, ctx->stream);
    if (so) launch_batch_publish(make_pub(done, g->h_out, g->d_sums, so), ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    for (size_t j = 0; j < count; j++) {
        const size_t i = tables[j];
        g->cur[i] = g->d_out[g->parity[i] & 1] + g->out_off[i];
        g->len[i] >>= ks[j];
        g->parity[i]++;
    }
    if (so) {
        CHK(wait_published(ctx, done));
        memcpy(next_sums, g->h_out, so * 8);
    }
    return ZIGZ_OK;
}

zigz_status gpu_batch_read_tail(void *user, size_t count, const size_t *tables, const size_t *ms, uint64_t *out) {
    GpuBatch *g = (GpuBatch *)user;
    zigz_ctx *ctx = g->ctx;
    BatchTab *d = (BatchTab *)(g->h_stage + g->tail_desc_off);
    size_t to = 0;
    unsigned wg = 0;
    for (size_t j = 0; j < count; j++) {
        const size_t i = tables[j];
        if (ms[j] != g->len[i]) return ZIGZ_ERR_PROTOCOL_ERROR;
        BatchTab b{};
        b.in = g->cur[i];
        b.log2_n = log2_floor(ms[j]);
        b.tail_off = to;
        b.first_wg = wg;
        d[j] = b;
        wg += (unsigned)((ms[j] + BATCH_WG - 1) / BATCH_WG);
        to += ms[j];
    }
    HIPCHK(ctx, hipMemcpyAsync(g->d_stage + g->tail_desc_off, d, count * sizeof(BatchTab), hipMemcpyHostToDevice, ctx->stream));
    const DoneFlag done = done_flag(ctx, 2);
    launch_batch_tails((const BatchTab *)(g->d_stage + g->tail_desc_off), (unsigned)count, wg,
                       make_pub(done, g->h_out, nullptr, to), ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    const uint32_t *h = (const uint32_t *)g->h_out;
    for (size_t x = 0; x < to; x++) out[x] = h[x];
    return ZIGZ_OK;
}

// the device batch after its arguments have been checked
zigz_status dev_batch_run(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k, const uint64_t *fixed,
                          uint64_t *rounds, uint64_t *points, uint64_t *final_evals) {
    ZIGZ_NOTHROW_BEGIN
    GpuBatch g;
    CHK(gpu_batch_init(ctx, g, k, d_tables, ns));
    const BatchOps ops{&g, gpu_batch_block_sums, gpu_batch_fold, gpu_batch_read_tail};
    return radix_run_batch(ops, k, ns, fixed, rounds, points, final_evals);
    ZIGZ_NOTHROW_END(ctx)
}

// what zigz_sumcheck_prove[_interactive] / zigz_dev_sumcheck_prove would say about table i before running it (the radix passes
// read 16-byte chunks)
zigz_status table_check(size_t n, const void *table, bool dev, const uint64_t *fixed) {
    return table_rule(TableRule{dev, false, true, false, 63}, &table, 1, n, fixed);
}

}  // namespace

extern "C" zigz_status zigz_sumcheck_radix_run_batch(void *user, zigz_radix_batch_sums_fn block_sums, zigz_radix_batch_fold_fn fold,
                                                     zigz_radix_batch_tail_fn read_tail, size_t k, const size_t *ns,
                                                     const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *points,
                                                     uint64_t *final_evals) {
    if (k == 0) return ZIGZ_OK;
    if (!block_sums || !fold || !read_tail || !ns || !rounds || !points || !final_evals || k > ZIGZ_BATCH_MAX)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    for (size_t i = 0, off = 0; i < k; i++) {
        CHK(mle_check(ns[i]));
        if (ns[i] == 1) return ZIGZ_ERR_NO_VARIABLES;
        if (fixed_challenges && !canonical(fixed_challenges + off, log2_floor(ns[i]))) return ZIGZ_ERR_NOT_CANONICAL;
        off += log2_floor(ns[i]);
    }
    ZIGZ_NOTHROW_BEGIN
    return radix_run_batch(BatchOps{user, block_sums, fold, read_tail}, k, ns, fixed_challenges, rounds, points, final_evals);
    ZIGZ_NOTHROW_END(nullptr)
}

extern "C" zigz_status zigz_dev_sumcheck_prove_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k,
                                                     const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *points,
                                                     uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !d_tables || !ns || !rounds || !points || !final_evals) return ZIGZ_ERR_INVALID_ARGUMENT;
    for (size_t i = 0, off = 0; i < k; i++) {
        const zigz_status st = table_check(ns[i], d_tables[i], true, fixed_challenges ? fixed_challenges + off : nullptr);
        if (st != ZIGZ_OK) return fail_at(bad_index, i, st);
        off += log2_floor(ns[i]);
    }
    return dev_batch_run(ctx, d_tables, ns, k, fixed_challenges, rounds, points, final_evals);
}

extern "C" zigz_status zigz_sumcheck_prove_batch(zigz_ctx *ctx, const uint64_t *const *tables, const size_t *ns, size_t k,
                                                 const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *points,
                                                 uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !tables || !ns || !rounds || !points || !final_evals) return ZIGZ_ERR_INVALID_ARGUMENT;
    ZIGZ_NOTHROW_BEGIN
    CHK(checks_in_call_order(tables, ns, k, bad_index, [&](size_t *f) -> zigz_status {
        for (size_t i = 0, off = 0; i < k; i++) {
            // (a non-power-of-two length fails before anything reads the table; a bad challenge only after the upload has checked
            // the values -- both are NOT_CANONICAL at the same table then)
            const zigz_status st = table_check(ns[i], tables[i], false, fixed_challenges ? fixed_challenges + off : nullptr);
            if (st != ZIGZ_OK) return fail_at(f, i, st);
            off += log2_floor(ns[i]);
        }
        return ZIGZ_OK;
    }));
    // one upload of all tables (each 16-byte aligned in the workspace), one range check
    const std::vector<size_t> at = packed_offsets(ns, k);
    std::vector<uint64_t> packed(at[k], 0);
    for (size_t i = 0; i < k; i++) memcpy(packed.data() + at[i], tables[i], ns[i] * 8);
    void *d32;
    CHK(ws_get(ctx, WS_SCBATCH_IN, at[k] * 4, &d32));
    const zigz_status up = upload_u64(ctx, packed.data(), at[k], (uint32_t *)d32, false);
    if (up == ZIGZ_ERR_NOT_CANONICAL) {
        for (size_t i = 0; i < k; i++)
            if (!canonical(tables[i], ns[i])) return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
    }
    CHK(up);
    std::vector<const uint32_t *> d(k);
    for (size_t i = 0; i < k; i++) d[i] = (const uint32_t *)d32 + at[i];
    return dev_batch_run(ctx, d.data(), ns, k, fixed_challenges, rounds, points, final_evals);
    ZIGZ_NOTHROW_END(ctx)
}

// ------------------------------------------------------------------ Lasso, batched (lasso_prover.zig:103-205)
namespace {
// what zigz_lasso_prove[_with_mapping] returns for instance `I` before its upload (pre) and after it (post)
zigz_status lasso_pre(const LassoInst &I) {
    const size_t w = I.n_in + I.n_out;
    if (I.mapping) CHK(lasso_mapping_check(I.table, I.table_rows, I.queries, I.n_queries, w, I.mapping, I.n_mapping));
    if (I.n_queries == 0) return ZIGZ_ERR_NO_QUERIES;  // :108-110
    if (!I.table || !I.queries || w == 0) return ZIGZ_ERR_INVALID_ARGUMENT;
    CHK(mle_check(I.table_rows));  // :124
    if (I.n_queries > ((size_t)1 << 40)) return ZIGZ_ERR_TOO_MANY_QUERIES;
    return ZIGZ_OK;
}
zigz_status lasso_post(const LassoInst &I, const LassoOut &o) {
    if (ceil_pow2(I.n_queries) == 1) return ZIGZ_ERR_NO_VARIABLES;  // :160
    if (!o.rounds || !o.point) return ZIGZ_ERR_INVALID_ARGUMENT;
    return ZIGZ_OK;
}
bool lasso_canonical(const LassoInst &I) {
    const size_t w = I.n_in + I.n_out;
    return canonical(I.table, I.table_rows * w) && canonical(I.queries, I.n_queries * w);
}
}  // namespace

extern "C" zigz_status zigz_lasso_prove_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *table_rows,
                                              const uint64_t *const *queries, const size_t *n_queries, const size_t *n_in,
                                              const size_t *n_out, const uint64_t *const *mappings, const size_t *n_mappings,
                                              size_t *nv_out, uint64_t *const *rounds, uint64_t *const *points, uint64_t *final_evals,
                                              uint8_t *query_commitments, uint8_t *table_commitments, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    if (k > ZIGZ_BATCH_MAX || !tables || !table_rows || !queries || !n_queries || !n_in || !n_out || (mappings && !n_mappings) ||
        !nv_out || !rounds || !points || !final_evals || !query_commitments || !table_commitments)
        return ZIGZ_ERR_INVALID_ARGUMENT;
    std::vector<LassoInst> inst_v;
    std::vector<LassoOut> out_v;
    ZIGZ_NOTHROW_BEGIN
    inst_v.resize(k);
    out_v.resize(k);
    ZIGZ_NOTHROW_END(ctx)
    for (size_t i = 0; i < k; i++) {
        const bool m = mappings && mappings[i];
        inst_v[i] = LassoInst{tables[i], table_rows[i], queries[i], n_queries[i], n_in[i], n_out[i], m ? mappings[i] : nullptr,
                              m ? n_mappings[i] : 0};
        out_v[i] = LassoOut{rounds[i], points[i]};
    }
    const LassoInst *inst = inst_v.data();
    const LassoOut *out = out_v.data();
    size_t f = k;
    zigz_status fst = ZIGZ_OK;
    bool post = false;  // the first failure is one the single call finds after its upload
    for (size_t i = 0; i < k && f == k; i++) {
        zigz_status st = lasso_pre(inst[i]);
        if (st == ZIGZ_OK) {
            st = lasso_post(inst[i], out[i]);
            post = st != ZIGZ_OK;
        }
        if (st != ZIGZ_OK) { f = i; fst = st; }
    }
    if (f < k) {
        for (size_t i = 0; i < f + (post ? 1 : 0); i++)
            if (!lasso_canonical(inst[i])) return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        return fail_at(bad_index, f, fst);
    }
    std::vector<uint32_t> h_fp;  // declared before the thread that reads it: destroyed after the join below
    std::vector<const uint32_t *> ev(2 * k);
    std::vector<size_t> evn(2 * k);
    std::vector<std::array<uint8_t, 32>> commits(2 * k);
    std::thread th;
    struct Joiner {
        std::thread &t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    } joiner{th};
    ZIGZ_NOTHROW_BEGIN
    // layout: rows (u64 host image, then u32 in the workspace) instance by instance, table then queries; fingerprints: table
    // fingerprints | query fingerprints padded to ceilPow2 (each query set 16-byte aligned: the sumcheck reads it in place)
    std::vector<size_t> row_at(2 * k + 1, 0), fp_at(2 * k + 1, 0);
    for (size_t i = 0; i < k; i++) {
        const size_t w = inst[i].n_in + inst[i].n_out;
        row_at[2 * i + 1] = row_at[2 * i] + inst[i].table_rows * w;
        row_at[2 * i + 2] = row_at[2 * i + 1] + inst[i].n_queries * w;
        fp_at[2 * i + 1] = (fp_at[2 * i] + inst[i].table_rows + 3) & ~(size_t)3;
        fp_at[2 * i + 2] = (fp_at[2 * i + 1] + ceil_pow2(inst[i].n_queries) + 3) & ~(size_t)3;
    }
    const size_t nrows = row_at[2 * k], nfp = fp_at[2 * k];
    void *d64, *d32, *dfp, *dtab;
    CHK(ws_get(ctx, WS_IN64, nrows * 8, &d64));
    CHK(ws_get(ctx, WS_IN32, nrows * 4, &d32));
    CHK(ws_get(ctx, WS_LASSO, nfp * 4, &dfp));
    CHK(ws_get(ctx, WS_MISC, 2 * k * sizeof(FpTab), &dtab));
    // one upload: every instance's rows into one image, one range check over all of it
    for (size_t i = 0; i < k; i++) {
        const size_t w = inst[i].n_in + inst[i].n_out;
        HIPCHK(ctx, hipMemcpyAsync((uint64_t *)d64 + row_at[2 * i], inst[i].table, inst[i].table_rows * w * 8,
                                   hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync((uint64_t *)d64 + row_at[2 * i + 1], inst[i].queries, inst[i].n_queries * w * 8,
                                   hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->d_flag, 0, 4, ctx->stream));
    launch_narrow_u64((const uint64_t *)d64, (uint32_t *)d32, nrows, ctx->d_flag, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    // one fingerprint launch over all tables and query sets (descriptors staged in pinned memory, copied once)
    FpTab *ht = (FpTab *)ctx->h_pin;
    if (2 * k * sizeof(FpTab) + 64 > PIN_WORDS * 8) return ZIGZ_ERR_INVALID_ARGUMENT;
    unsigned wg = 0;
    for (size_t s = 0; s < 2 * k; s++) {
        const LassoInst &I = inst[s / 2];
        const bool q = s & 1;
        FpTab t{};
        t.in = (const uint32_t *)d32 + row_at[s];
        t.out = (uint32_t *)dfp + fp_at[s];
        t.rows = q ? I.n_queries : I.table_rows;
        t.padded = q ? ceil_pow2(I.n_queries) : I.table_rows;  // zero-pad, :139-142
        t.width = (uint32_t)(I.n_in + I.n_out);
        t.first_wg = wg;
        ht[s] = t;
        wg += (unsigned)((t.padded + BATCH_WG - 1) / BATCH_WG);
    }
    uint32_t *hflag = (uint32_t *)(ctx->h_pin + PIN_WORDS - 8);
    HIPCHK(ctx, hipMemcpyAsync(hflag, ctx->d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dtab, ht, 2 * k * sizeof(FpTab), hipMemcpyHostToDevice, ctx->stream));
    launch_batch_fingerprints((const FpTab *)dtab, (unsigned)(2 * k), wg, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    // all fingerprints in one copy
    h_fp.resize(nfp);
    HIPCHK(ctx, hipMemcpyAsync(h_fp.data(), dfp, nfp * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (*hflag) {
        set_err(ctx, "%s", NOT_CANONICAL_TEXT);
        for (size_t i = 0; i < k; i++)
            if (!lasso_canonical(inst[i])) return fail_at(bad_index, i, ZIGZ_ERR_NOT_CANONICAL);
        return ZIGZ_ERR_NOT_CANONICAL;
    }
    // the 2k flat commitments (commitToPolynomial, :242-252) on the host, underneath the GPU sumcheck
    for (size_t s = 0; s < 2 * k; s++) {
        const LassoInst &I = inst[s / 2];
        ev[s] = h_fp.data() + fp_at[s];
        evn[s] = (s & 1) ? ceil_pow2(I.n_queries) : I.table_rows;
    }
    th = std::thread([&ev, &evn, &commits, k] {
        flat_commit_batch(ev.data(), evn.data(), 2 * k, reinterpret_cast<uint8_t(*)[32]>(commits.data()));
    });
    // the batched sumcheck over the query fingerprints, in place
    std::vector<const uint32_t *> dq(k);
    std::vector<size_t> nq(k), voff(k + 1, 0);
    for (size_t i = 0; i < k; i++) {
        dq[i] = (const uint32_t *)dfp + fp_at[2 * i + 1];
        nq[i] = ceil_pow2(inst[i].n_queries);
        voff[i + 1] = voff[i] + log2_floor(nq[i]);
    }
    std::vector<uint64_t> sc_rounds(2 * voff[k]), sc_points(voff[k]), fe(k);
    CHK(dev_batch_run(ctx, dq.data(), nq.data(), k, nullptr, sc_rounds.data(), sc_points.data(), fe.data()));
    th.join();
    for (size_t i = 0; i < k; i++) {
        const size_t v = voff[i + 1] - voff[i];
        nv_out[i] = v;
        memcpy(out[i].rounds, sc_rounds.data() + 2 * voff[i], 2 * v * 8);
        memcpy(out[i].point, sc_points.data() + voff[i], v * 8);
        final_evals[i] = fe[i];
        memcpy(table_commitments + 32 * i, commits[2 * i].data(), 32);
        memcpy(query_commitments + 32 * i, commits[2 * i + 1].data(), 32);
    }
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}
