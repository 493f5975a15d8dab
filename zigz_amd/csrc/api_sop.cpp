// C ABI of libzigz_hip.so, part 10: the batched sum-of-products sumcheck prover and its verifier.  The schedule
// and the verifier are product_schedule.hpp's; here: what the sop family hands them -- pools instead of factor lists (every POOL
// table is loaded, bound and stored once per round, whatever number of terms names it: 2 M n bytes of bound copies per instance),
// class sums to c_0..c_D (sop_host.hpp: coefficients), sop_host.hpp's tail rounds and verdict, eq entries as closed forms -- and
// the four entries.
#include "product_schedule.hpp"

using namespace zk;

static_assert(sop::MAX_TABLES == SOP_MAX_TABLES && sop::MAX_TERMS == SOP_MAX_TERMS && sop::SUMS == SOP_SUMS, "header, host and kernels");
static_assert(sop::CLASS_AT[0] == SOP_CLASS_AT[0] && sop::CLASS_AT[1] == SOP_CLASS_AT[1] && sop::CLASS_AT[2] == SOP_CLASS_AT[2],
              "the host reads the class sums where the kernels write them");
static_assert(sop::MAX_DEGREE == PRODUCT_MAX_DEGREE && pd::R1 == R_MOD_P, "the host's scales are powers of the kernels' R");

namespace {

struct Sop : sched::PoolTerms {
    static constexpr size_t BEHIND = 0;
    uint64_t *table_evals, *final_evals;

    Sop(const sop::Args &a, uint64_t *table_evals, uint64_t *final_evals)
        : PoolTerms(a), table_evals(table_evals), final_evals(final_evals) {}
    unsigned ncoef(size_t i) const { return sh[i].D + 1; }
    size_t payload_words(size_t) const { return 0; }
    void payload(size_t, uint32_t *) const {}
    void behind(size_t, void *, const uint32_t *, size_t, bool) const {}
    void sums(const SopTab *d, unsigned n, unsigned wg, unsigned long long *part, hipStream_t s) const { launch_sop_sums(d, n, wg, part, s); }
    void bind(const SopTab *d, unsigned n, unsigned wg, unsigned long long *part, hipStream_t s) const { launch_sop_bind(d, n, wg, part, s); }
    uint64_t step(size_t i, SumcheckRounds &pr, const uint64_t *sums) const {
        uint64_t c[SOP_SUMS];
        sop::coefficients(sh[i].D, sums, c);
        return pr.step(c);
    }
    void finish_tail(size_t i, SumcheckRounds &pr, std::vector<uint64_t> *f) const {
        final_evals[i] = sop::tail_rounds(pr, f, sh[i].M, sh[i].terms, sh[i].T, table_evals + sh[i].moff);
    }
};

zigz_status run(zigz_ctx *ctx, const sop::Args &a, const uint32_t *const *d_tables, const uint64_t *const *h_tables,
                uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points, uint64_t *table_evals, uint64_t *final_evals,
                size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    Sop fam(a, table_evals, final_evals);
    return sched::run(ctx, fam, a.k, d_tables, h_tables, a.ns, a.fixed, claimed_sums, rounds, points, bad_index);
    ZIGZ_NOTHROW_END(ctx)
}

// the verifier's entry: a pool entry is a table or eq(tau, .), whose taus follow one another in eq_points
struct SopVerify {
    const sop::VerifyArgs &a;
    const std::vector<sop::Shape> &sh;
    std::vector<size_t> eoff;  // per proof: its first tau word

    SopVerify(const sop::VerifyArgs &a, const std::vector<sop::Shape> &sh) : a(a), sh(sh), eoff(a.k + 1, 0) {
        for (size_t i = 0; i < a.k; i++) {
            size_t neq = 0;
            for (unsigned j = 0; j < sh[i].M; j++) neq += !is_pair(sh[i].moff + j);
            eoff[i + 1] = eoff[i] + neq * sh[i].nv;
        }
    }
    bool is_pair(size_t e) const { return sop::kind_of(a, e) != pv::KIND_EQ; }
    unsigned degree(size_t i) const { return sh[i].D; }
    size_t roff(size_t i) const { return sh[i].roff; }
    void host_values(size_t i, bool reversed, uint64_t *ev) const {
        const uint64_t *tau = a.eq_points ? a.eq_points + eoff[i] : nullptr;
        for (unsigned j = 0; j < sh[i].M; j++)
            if (!is_pair(sh[i].moff + j)) {
                ev[j] = pv::eq_at(tau, a.points + sh[i].voff, sh[i].nv, reversed);
                tau += sh[i].nv;
            }
    }
    uint8_t verdict(size_t i, const sv::Replay &rep, const uint64_t *ev) const {
        return sop::verdict(rep, sh[i].terms, sh[i].T, ev, sh[i].M, a.final_evals[i], a.table_evals ? a.table_evals + sh[i].moff : nullptr);
    }
};

zigz_status verify(zigz_ctx *ctx, const sop::VerifyArgs &a, bool host_tables, uint8_t *verdicts, uint64_t *expected_evals,
                   uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    if (a.k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    ZIGZ_NOTHROW_BEGIN
    const std::vector<sop::Shape> sh = sop::shapes(a.k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs);
    SopVerify entry(a, sh);
    return sched::verify_pool(ctx, a, sh, entry, host_tables, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_dev_sumcheck_prove_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables,
                                                         const uint32_t *const *d_tables, const size_t *ns, const unsigned *n_terms,
                                                         const unsigned *term_degrees, const uint8_t *term_tables,
                                                         const uint64_t *term_coeffs, const uint64_t *fixed_challenges,
                                                         uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points,
                                                         uint64_t *table_evals, uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const sop::Args a{k, n_tables, (const void *const *)d_tables, ns, n_terms, term_degrees, term_tables, term_coeffs, fixed_challenges,
                      claimed_sums, rounds, points, table_evals, final_evals};
    CHK(sop::check_sop_batch(a, true, false, bad_index));
    return run(ctx, a, d_tables, nullptr, claimed_sums, rounds, points, table_evals, final_evals, bad_index);
}

extern "C" zigz_status zigz_sumcheck_prove_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                     const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                     const uint8_t *term_tables, const uint64_t *term_coeffs,
                                                     const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                     uint64_t *points, uint64_t *table_evals, uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const sop::Args a{k, n_tables, (const void *const *)tables, ns, n_terms, term_degrees, term_tables, term_coeffs, fixed_challenges,
                      claimed_sums, rounds, points, table_evals, final_evals};
    ZIGZ_NOTHROW_BEGIN
    CHK(host_value_checks(ctx, [&](bool *value) { return sop::check_sop_batch_host(a, bad_index, value); }));
    ZIGZ_NOTHROW_END(ctx)
    return run(ctx, a, nullptr, tables, claimed_sums, rounds, points, table_evals, final_evals, bad_index);
}

extern "C" zigz_status zigz_dev_sumcheck_verify_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables,
                                                          const uint32_t *const *d_tables, const uint8_t *table_kinds,
                                                          const uint64_t *eq_points, const size_t *ns, const unsigned *n_terms,
                                                          const unsigned *term_degrees, const uint8_t *term_tables,
                                                          const uint64_t *term_coeffs, const uint64_t *claimed_sums,
                                                          const uint64_t *rounds, const uint64_t *points, const uint64_t *table_evals,
                                                          const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                                          uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                          size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const sop::VerifyArgs a{k, n_tables, (const void *const *)d_tables, table_kinds, eq_points, ns, n_terms, term_degrees, term_tables,
                            term_coeffs, claimed_sums, rounds, points, table_evals, final_evals, flags, n_rejected};
    CHK(sop::check_verify_sop_batch(a, true, false, bad_index));
    return verify(ctx, a, false, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_sumcheck_verify_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                      const uint8_t *table_kinds, const uint64_t *eq_points, const size_t *ns,
                                                      const unsigned *n_terms, const unsigned *term_degrees, const uint8_t *term_tables,
                                                      const uint64_t *term_coeffs, const uint64_t *claimed_sums, const uint64_t *rounds,
                                                      const uint64_t *points, const uint64_t *table_evals, const uint64_t *final_evals,
                                                      uint32_t flags, uint8_t *verdicts, uint64_t *expected_evals,
                                                      uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const sop::VerifyArgs a{k, n_tables, (const void *const *)tables, table_kinds, eq_points, ns, n_terms, term_degrees, term_tables,
                            term_coeffs, claimed_sums, rounds, points, table_evals, final_evals, flags, n_rejected};
    CHK(host_value_checks(ctx, [&](bool *value) { return sop::check_verify_sop_batch_host(a, bad_index, value); }));
    return verify(ctx, a, true, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}
