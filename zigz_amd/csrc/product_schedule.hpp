#pragma once
// The round schedule of the batched product, sum-of-products and zero-check provers (api_product.cpp, api_sop.cpp,
// api_zerocheck.cpp), once, and the verifier of the two pool families.
//
// Schedule of one call.  Instances longer than 1024 are LIVE.  Round 0: the host writes the live instances' descriptors into
// pinned memory and queues one copy of them, one launch that sums every live instance's round-0 terms over the caller's tables
// and one small launch that reduces them into pinned memory and stores the completion word; the host polls that word, turns
// the sums into coefficients and steps every live transcript on its threads.  Every later round is the same copy and two
// launches with the fused bind pass in place of the sums (the first one writes each table's bound copy, n/2 words, into the
// workspace; the later ones run in place there); an instance leaves the live set when its tables are 1024 long.  One launch
// then hands the current tables of ALL instances to the host, which finishes their rounds.  The workspaces are one set for the
// three families: calls on a context are serial.
//
// A family describes what is its own:
//   Tab, SUMS, MAX_TABLES   its descriptor, the result words per instance, the most tables an instance has
//   BEHIND                  bytes that follow every descriptor in a round's copy (zero-check: the instance's ZcWeights)
//   n_tables(i), ncoef(i)   instance i's tables; its coefficients per round, which are also its round words' stride
//   describe(i, p)          the descriptor's own fields (the schedule writes in, out, m, r_m, first_wg, slot and tail_off)
//   payload_words(n)        a live instance's words in the payload the FIRST copy carries behind the descriptors, and
//   payload(i, h)           ... those words (zero-check: the weights, which stay where they are for the rest of the call)
//   behind(i, h, d, m, b)   what follows descriptor i in a pass over tables of m values (b: a bind pass); d: its payload on the device
//   sums, bind, finish, tails   its launches
//   step(i, pr, sums)       one round from the published sums: coefficients, transcript, challenge
//   finish_tail(i, pr, f)   the last rounds on the host from the instance's tail tables, and its outputs
//
// The verifier replays the rounds on the host's threads while the batched eval's launch (api_mle_batch.cpp) evaluates every table
// entry of every pool once; eq values are closed forms on the host; the entry's verdict combines them through the terms.
#include "api_internal.hpp"
#include "sop_host.hpp"

namespace sched {

template <unsigned MAX_TABLES>
struct Inst {
    size_t len = 0, tail_off = 0;
    size_t pay_off = 0;  // live: first word of its payload in the payload region
    const uint32_t *cur[MAX_TABLES] = {};
    uint32_t *work[MAX_TABLES] = {};
    uint64_t ch = 0;  // the challenge of the instance's last round
    SumcheckRounds pr;
};

// one call's pinned region: sums (SUMS u64 per instance) | tails (u32) | round descriptors and what goes behind them | payload |
// tail descriptors | the narrowed tables of the host form.  The device staging holds descriptors | payload | tail descriptors |
// partials.
struct Layout {
    size_t tail_off = 0, tail_words = 0, desc_off = 0, desc_bytes = 0, pay_off = 0, pay_bytes = 0, tdesc_off = 0, tdesc_bytes = 0,
           tab_off = 0, tab_words = 0, bytes = 0;
    size_t nwg = 0, work_words = 0;  // workgroups of round 0; words of all bound copies
    std::vector<size_t> fns, owner;  // every table's length and instance
    std::vector<size_t> at;          // host form: table f's first word among the narrowed tables (each 16-byte aligned)
};

template <class F>
zigz_status plan(const F &fam, size_t k, const size_t *ns, bool host_tables, Layout &L) {
    size_t pay_words = 0;
    for (size_t i = 0; i < k; i++) {
        const unsigned M = fam.n_tables(i);
        L.tail_words += M * (ns[i] < HOST_TAIL_MAX ? ns[i] : HOST_TAIL_MAX);
        if (ns[i] > HOST_TAIL_MAX) {
            L.nwg += product_wgs(ns[i]);
            L.work_words += M * (ns[i] / 2);
            pay_words += fam.payload_words(ns[i]);
        }
        L.fns.insert(L.fns.end(), M, ns[i]);
        L.owner.insert(L.owner.end(), M, i);
    }
    if (L.nwg > MLE_BATCH_MAX_WGS) return ZIGZ_ERR_INVALID_ARGUMENT;  // one launch: fewer than 2^32 threads in its grid
    L.desc_bytes = align256(k * (sizeof(typename F::Tab) + F::BEHIND));
    L.pay_bytes = align256(pay_words * 4);
    L.tdesc_bytes = align256(k * sizeof(typename F::Tab));
    L.tail_off = align256(k * F::SUMS * 8);
    L.desc_off = L.tail_off + align256(L.tail_words * 4);
    L.pay_off = L.desc_off + L.desc_bytes;
    L.tdesc_off = L.pay_off + L.pay_bytes;
    L.tab_off = L.tdesc_off + L.tdesc_bytes;
    if (host_tables) {
        L.at = packed_offsets(L.fns.data(), L.fns.size());
        L.tab_words = L.at[L.fns.size()];
    }
    L.bytes = L.tab_off + L.tab_words * 4;
    return ZIGZ_OK;
}

// d_tables or h_tables: every instance's tables one behind the other, on the device or on the host.  transcripts (k of them, or
// none: a fresh one per instance): the transcript instance i starts from, handed back as its last round left it -- a caller
// whose proof runs through several calls (api_grand_product.cpp: one call per layer) carries it from one to the next
template <class F>
zigz_status run(zigz_ctx *ctx, F &fam, size_t k, const uint32_t *const *d_tables, const uint64_t *const *h_tables, const size_t *ns,
                const uint64_t *fixed, uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points, size_t *bad_index,
                Transcript *transcripts = nullptr) {
    using Tab = typename F::Tab;
    ZIGZ_NOTHROW_BEGIN
    Layout L;
    CHK(plan(fam, k, ns, h_tables != nullptr, L));
    uint8_t *pin;
    CHK(pinned(ctx, L.bytes, &pin));
    std::vector<const uint32_t *> up;
    if (h_tables) {
        CHK(stage_host_tables(ctx, h_tables, L.fns.data(), L.fns.size(), L.at, (uint32_t *)(pin + L.tab_off), WS_PRODUCT_IN,
                              L.owner.data(), up, bad_index));
        d_tables = up.data();
    }
    void *d_stage, *d_work;
    CHK(ws_get(ctx, WS_PRODUCT, L.desc_bytes + L.pay_bytes + L.tdesc_bytes + L.nwg * F::SUMS * 8, &d_stage));
    CHK(ws_get(ctx, WS_PRODUCT_WORK, L.work_words * 4, &d_work));
    const Tab *d_desc = (const Tab *)d_stage, *d_tdesc = (const Tab *)((uint8_t *)d_stage + L.desc_bytes + L.pay_bytes);
    const uint32_t *d_pay = (const uint32_t *)((uint8_t *)d_stage + L.desc_bytes);
    unsigned long long *d_part = (unsigned long long *)((uint8_t *)d_stage + L.desc_bytes + L.pay_bytes + L.tdesc_bytes);
    Tab *h_desc = (Tab *)(pin + L.desc_off), *h_tdesc = (Tab *)(pin + L.tdesc_off);
    uint32_t *h_pay = (uint32_t *)(pin + L.pay_off);
    const uint64_t *h_sums = (const uint64_t *)pin;

    std::vector<Inst<F::MAX_TABLES>> t(k);
    std::vector<size_t> live, next;
    {
        size_t foff = 0, voff = 0, roff = 0, woff = 0, toff = 0, poff = 0;
        for (size_t i = 0; i < k; i++) {
            auto &s = t[i];
            const unsigned M = fam.n_tables(i);
            s.len = ns[i];
            s.tail_off = toff;
            toff += M * (ns[i] < HOST_TAIL_MAX ? ns[i] : HOST_TAIL_MAX);
            for (unsigned j = 0; j < M; j++) {
                s.cur[j] = d_tables[foff + j];
                if (ns[i] > HOST_TAIL_MAX) {  // every table's bound copy is 16-byte aligned: n / 2 >= 1024 words
                    s.work[j] = (uint32_t *)d_work + woff;
                    woff += ns[i] / 2;
                }
            }
            s.pr.ncoef = fam.ncoef(i);
            s.pr.nv = log2_floor(ns[i]);
            s.pr.claimed_sum = claimed_sums + i;
            s.pr.rounds = rounds + roff;
            s.pr.point = points + voff;
            s.pr.fixed = fixed ? fixed + voff : nullptr;
            if (transcripts) s.pr.tr = transcripts[i];
            foff += M;
            voff += s.pr.nv;
            roff += (size_t)s.pr.ncoef * s.pr.nv;
            if (ns[i] > HOST_TAIL_MAX) {
                s.pay_off = poff;
                poff += fam.payload_words(ns[i]);
                live.push_back(i);
            }
        }
    }
    // the live instances' payload, behind the descriptors of the first copy
    if (L.pay_bytes) parallel_for(live.size(), [&](size_t x) { fam.payload(live[x], h_pay + t[live[x]].pay_off); });
    // instance i's descriptor with its current tables
    auto describe = [&](size_t i) {
        Tab p{};
        for (unsigned j = 0; j < fam.n_tables(i); j++) p.in[j] = t[i].cur[j];
        p.m = t[i].len;
        fam.describe(i, p);
        return p;
    };
    // the live instances' descriptors, and what goes behind them, for one pass; returns its workgroup count
    auto fill = [&](bool bind) {
        unsigned wg = 0;
        uint8_t *h_behind = (uint8_t *)(h_desc + live.size());
        for (size_t x = 0; x < live.size(); x++) {
            const auto &s = t[live[x]];
            Tab p = describe(live[x]);
            for (unsigned j = 0; bind && j < fam.n_tables(live[x]); j++) p.out[j] = s.work[j];
            p.r_m = bind ? host_to_mont(s.ch) : 0;
            p.first_wg = wg;
            p.slot = (uint32_t)live[x];
            h_desc[x] = p;
            fam.behind(live[x], h_behind + x * F::BEHIND, d_pay + s.pay_off, s.len, bind);
            wg += (unsigned)product_wgs(s.len);
        }
        return wg;
    };
    // the round of the instances in `who` from the published sums; every transcript steps on a thread of its own
    auto step = [&](const std::vector<size_t> &who) {
        parallel_for(who.size(), [&](size_t x) { t[who[x]].ch = fam.step(who[x], t[who[x]].pr, h_sums + F::SUMS * who[x]); });
    };
    if (!live.empty()) {  // round 0: sums over the caller's tables; the copy carries the payload too
        const unsigned wg = fill(false);
        const size_t bytes = L.pay_bytes ? L.desc_bytes + L.pay_bytes : live.size() * (sizeof(Tab) + F::BEHIND);
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_desc, bytes, hipMemcpyHostToDevice, ctx->stream));
        const DoneFlag done = done_flag(ctx, 2);
        fam.sums(d_desc, (unsigned)live.size(), wg, d_part, ctx->stream);
        fam.finish(d_desc, (unsigned)live.size(), d_part, (uint64_t *)pin, ctx->stream, done);
        HIPCHK(ctx, hipGetLastError());
        CHK(wait_published(ctx, done));
        step(live);
    }
    // A later round: bind with the last challenge, sum the next round's terms.  (No transcript's status is looked at in between: a
    // step fails only on a fixed challenge >= p, and every entry's checks have rejected those before anything ran --
    // sumcheck_host.hpp: table_rule takes the fixed challenges as the instance's words.  The one look at the end is enough.)
    while (!live.empty()) {
        const unsigned wg = fill(true);
        next.clear();
        for (size_t i : live) {
            auto &s = t[i];
            for (unsigned j = 0; j < fam.n_tables(i); j++) s.cur[j] = s.work[j];
            s.len /= 2;
            if (s.len > HOST_TAIL_MAX) next.push_back(i);
        }
        HIPCHK(ctx, hipMemcpyAsync(d_stage, h_desc, live.size() * (sizeof(Tab) + F::BEHIND), hipMemcpyHostToDevice, ctx->stream));
        fam.bind(d_desc, (unsigned)live.size(), wg, d_part, ctx->stream);
        if (!next.empty()) {  // (an instance that is 1024 long now has its next round on the host: nobody reads its sums)
            const DoneFlag done = done_flag(ctx, 2);
            fam.finish(d_desc, (unsigned)live.size(), d_part, (uint64_t *)pin, ctx->stream, done);
            HIPCHK(ctx, hipGetLastError());
            CHK(wait_published(ctx, done));
            step(next);
        } else {
            HIPCHK(ctx, hipGetLastError());
        }
        live.swap(next);
    }
    // every instance's current tables in one hand-off
    for (size_t i = 0; i < k; i++) {
        Tab p = describe(i);
        p.tail_off = t[i].tail_off;
        h_tdesc[i] = p;
    }
    HIPCHK(ctx, hipMemcpyAsync((void *)d_tdesc, h_tdesc, k * sizeof(Tab), hipMemcpyHostToDevice, ctx->stream));
    const DoneFlag done = done_flag(ctx, 2);
    fam.tails(d_tdesc, (unsigned)k, (uint32_t *)(pin + L.tail_off), ctx->stream, done);
    HIPCHK(ctx, hipGetLastError());
    CHK(wait_published(ctx, done));
    const uint32_t *h_tail = (const uint32_t *)(pin + L.tail_off);
    for (size_t x = 0; x < L.tail_words; x++)
        if (h_tail[x] >= P) {  // (a device table is not checked on the way in)
            set_err(ctx, "%s", NOT_CANONICAL_TEXT);
            return ZIGZ_ERR_NOT_CANONICAL;
        }
    parallel_for(k, [&](size_t i) {
        auto &s = t[i];
        std::vector<uint64_t> f[F::MAX_TABLES];
        for (unsigned j = 0; j < fam.n_tables(i); j++) f[j].assign(h_tail + s.tail_off + j * s.len, h_tail + s.tail_off + (j + 1) * s.len);
        fam.finish_tail(i, s.pr, f);
    });
    for (const auto &s : t)
        if (s.pr.st != ZIGZ_OK) return s.pr.st;
    for (size_t i = 0; transcripts && i < k; i++) transcripts[i] = t[i].pr.tr;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

// What the sop and zero-check families share: the pool's descriptor, its terms sorted by degree as the kernels walk them
struct PoolTerms {
    using Tab = SopTab;
    static constexpr unsigned SUMS = SOP_SUMS, MAX_TABLES = SOP_MAX_TABLES;
    struct Sorted {
        SopTerm term[SOP_MAX_TERMS] = {};
        unsigned n_deg[PRODUCT_MAX_DEGREE] = {};
    };
    const std::vector<sop::Shape> sh;
    std::vector<Sorted> sorted;

    explicit PoolTerms(const sop::Args &a)
        : sh(sop::shapes(a.k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs)), sorted(a.k) {
        for (size_t i = 0; i < a.k; i++) {
            unsigned nt = 0;
            for (unsigned d = 1; d <= PRODUCT_MAX_DEGREE; d++)
                for (unsigned x = 0; x < sh[i].T; x++)
                    if (sh[i].terms[x].d == d) {
                        sorted[i].term[nt++] = SopTerm{sop_term_word(d, sh[i].terms[x].idx), host_to_mont(sh[i].terms[x].alpha)};
                        sorted[i].n_deg[d - 1]++;
                    }
        }
    }
    unsigned n_tables(size_t i) const { return sh[i].M; }
    void describe(size_t i, SopTab &p) const {
        for (unsigned x = 0; x < sh[i].T; x++) p.term[x] = sorted[i].term[x];
        p.n_tables = sh[i].M;
        p.n_terms = sh[i].T;
        p.n_d1 = sorted[i].n_deg[0];
        p.n_d2 = sorted[i].n_deg[1];
    }
    void finish(const SopTab *d, unsigned n, const unsigned long long *part, uint64_t *out, hipStream_t s, DoneFlag done) const {
        launch_sop_finish(d, n, part, out, s, done);
    }
    void tails(const SopTab *d, unsigned n, uint32_t *h_dst, hipStream_t s, DoneFlag done) const { launch_sop_tails(d, n, h_dst, s, done); }
};

// ---- verification of the pool families: the oracles are the pools' entries, a table (one pair of the eval launch) or a closed
// form on the host.  The entry supplies, over shapes `sh`:
//   is_pair(e)             pool entry e (counted over the whole batch) is a table
//   degree(i), roff(i)     the degree of proof i's round polynomials and its first round word
//   host_values(i, r, ev)  its closed forms, underneath the evaluation (ev: the proof's pool entries' evaluations; r: reversed)
//   verdict(i, rep, ev)    ... once ev holds the tables' evaluations too
template <class A, class E>
zigz_status verify_pool(zigz_ctx *ctx, const A &a, const std::vector<sop::Shape> &sh, E &entry, bool host_tables, uint8_t *verdicts,
                        uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    const size_t k = a.k;
    const bool reversed = (a.flags & ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED) != 0;
    // per pool entry: its pair of the eval launch, or none
    std::vector<const void *> tabs;
    std::vector<size_t> pair_ns, owner, pair_of;
    std::vector<uint64_t> pair_points;
    for (size_t i = 0; i < k; i++)
        for (unsigned j = 0; j < sh[i].M; j++) {
            if (!entry.is_pair(sh[i].moff + j)) {
                pair_of.push_back((size_t)-1);
                continue;
            }
            pair_of.push_back(tabs.size());
            tabs.push_back(a.tables[sh[i].moff + j]);
            pair_ns.push_back(a.ns[i]);
            owner.push_back(i);
            pair_points.insert(pair_points.end(), a.points + sh[i].voff, a.points + sh[i].voff + sh[i].nv);
        }
    const size_t m = tabs.size(), entries = pair_of.size();
    DoneFlag done;
    const uint64_t *pairs = nullptr;
    CHK(mle_eval_pairs_queue(ctx, tabs.data(), host_tables, pair_ns.data(), m, pair_points.data(), reversed, owner.data(), &pairs, &done,
                             bad_index));
    // the k replays and the closed forms, underneath the evaluation
    std::vector<sv::Replay> rep(k);
    std::vector<uint64_t> ev(entries, 0);
    parallel_for(k, [&](size_t i) {
        rep[i] = pv::replay_rounds(a.claimed_sums[i], a.rounds + entry.roff(i), sh[i].nv, entry.degree(i));
        entry.host_values(i, reversed, ev.data() + sh[i].moff);
    });
    if (m) CHK(wait_published(ctx, done));
    size_t rejected = 0;
    for (size_t i = 0; i < k; i++) {
        for (unsigned j = 0; j < sh[i].M; j++)
            if (pair_of[sh[i].moff + j] != (size_t)-1) ev[sh[i].moff + j] = pairs[pair_of[sh[i].moff + j]];
        const uint8_t ok = entry.verdict(i, rep[i], ev.data() + sh[i].moff);
        rejected += !ok;
        if (verdicts) verdicts[i] = ok;
        if (expected_evals) expected_evals[i] = rep[i].expected;
    }
    if (oracle_evals) memcpy(oracle_evals, ev.data(), entries * 8);
    *n_rejected = rejected;
    return ZIGZ_OK;
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace sched
