// C ABI of libzigz_hip.so, part 11: the zero-check sumcheck with the eq factor in closed form and its verifier.
// The schedule and the verifier are product_schedule.hpp's, over a pool WITHOUT eq; what the zero-check family hands the schedule
// is zerocheck_family.hpp's (the grand-product prover runs its layers through the same family); here: the entries and what the
// family hands the verifier.  eq(tau, q) is a closed form on the host, for the prover and the verifier.
#include "zerocheck_family.hpp"

using namespace zk;
using sched::ZeroCheck;

namespace {

zigz_status run(zigz_ctx *ctx, const zc::Args &za, const uint32_t *const *d_tables, const uint64_t *const *h_tables,
                uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals,
                uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_NOTHROW_BEGIN
    ZeroCheck fam(za, table_evals, eq_evals, final_evals);
    return sched::run(ctx, fam, za.s.k, d_tables, h_tables, za.s.ns, za.s.fixed, claimed_sums, rounds, points, bad_index);
    ZIGZ_NOTHROW_END(ctx)
}

// the verifier's entry: every pool entry is a table; eq(tau, q) is one closed form per proof
struct ZcVerify {
    const zc::VerifyArgs &a;
    const std::vector<sop::Shape> &sh;
    const std::vector<size_t> roffs;
    std::vector<uint64_t> eq;

    ZcVerify(const zc::VerifyArgs &a, const std::vector<sop::Shape> &sh) : a(a), sh(sh), roffs(zc::round_offsets(sh)), eq(a.k, 0) {}
    bool is_pair(size_t) const { return true; }
    unsigned degree(size_t i) const { return sh[i].D + 1; }
    size_t roff(size_t i) const { return roffs[i]; }
    void host_values(size_t i, bool reversed, uint64_t *) {
        eq[i] = pv::eq_at(a.eq_points + sh[i].voff, a.points + sh[i].voff, sh[i].nv, reversed);
    }
    uint8_t verdict(size_t i, const sv::Replay &rep, const uint64_t *ev) const {
        return zc::verdict(rep, sh[i].terms, sh[i].T, ev, sh[i].M, eq[i], a.final_evals[i],
                           a.table_evals ? a.table_evals + sh[i].moff : nullptr, a.eq_evals ? a.eq_evals + i : nullptr);
    }
};

zigz_status verify(zigz_ctx *ctx, const zc::VerifyArgs &a, bool host_tables, uint8_t *verdicts, uint64_t *expected_evals,
                   uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index) {
    if (a.k == 0) {
        *n_rejected = 0;
        return ZIGZ_OK;
    }
    ZIGZ_NOTHROW_BEGIN
    const std::vector<sop::Shape> sh = sop::shapes(a.k, a.n_tables, a.ns, a.n_terms, a.term_degrees, a.term_tables, a.term_coeffs);
    ZcVerify entry(a, sh);
    return sched::verify_pool(ctx, a, sh, entry, host_tables, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
    ZIGZ_NOTHROW_END(ctx)
}

}  // namespace

extern "C" zigz_status zigz_dev_sumcheck_prove_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables,
                                                               const uint32_t *const *d_tables, const size_t *ns, const unsigned *n_terms,
                                                               const unsigned *term_degrees, const uint8_t *term_tables,
                                                               const uint64_t *term_coeffs, const uint64_t *eq_points,
                                                               const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                               uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals,
                                                               uint64_t *final_evals, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const zc::Args a{{k, n_tables, (const void *const *)d_tables, ns, n_terms, term_degrees, term_tables, term_coeffs, fixed_challenges,
                      claimed_sums, rounds, points, table_evals, final_evals},
                     eq_points, eq_evals};
    CHK(zc::check_zerocheck_batch(a, true, false, bad_index));
    return run(ctx, a, d_tables, nullptr, claimed_sums, rounds, points, table_evals, eq_evals, final_evals, bad_index);
}

extern "C" zigz_status zigz_sumcheck_prove_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                           const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                           const uint8_t *term_tables, const uint64_t *term_coeffs,
                                                           const uint64_t *eq_points, const uint64_t *fixed_challenges,
                                                           uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points,
                                                           uint64_t *table_evals, uint64_t *eq_evals, uint64_t *final_evals,
                                                           size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    if (k == 0) return ZIGZ_OK;
    const zc::Args a{{k, n_tables, (const void *const *)tables, ns, n_terms, term_degrees, term_tables, term_coeffs, fixed_challenges,
                      claimed_sums, rounds, points, table_evals, final_evals},
                     eq_points, eq_evals};
    ZIGZ_NOTHROW_BEGIN
    CHK(host_value_checks(ctx, [&](bool *value) { return zc::check_zerocheck_batch_host(a, bad_index, value); }));
    ZIGZ_NOTHROW_END(ctx)
    return run(ctx, a, nullptr, tables, claimed_sums, rounds, points, table_evals, eq_evals, final_evals, bad_index);
}

extern "C" zigz_status zigz_dev_sumcheck_verify_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables,
                                                                const uint32_t *const *d_tables, const uint64_t *eq_points,
                                                                const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                                const uint8_t *term_tables, const uint64_t *term_coeffs,
                                                                const uint64_t *claimed_sums, const uint64_t *rounds,
                                                                const uint64_t *points, const uint64_t *table_evals,
                                                                const uint64_t *eq_evals, const uint64_t *final_evals, uint32_t flags,
                                                                uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                                size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const zc::VerifyArgs a{k, n_tables, (const void *const *)d_tables, eq_points, ns, n_terms, term_degrees, term_tables, term_coeffs,
                           claimed_sums, rounds, points, table_evals, eq_evals, final_evals, flags, n_rejected};
    CHK(zc::check_verify_zerocheck_batch(a, true, false, bad_index));
    return verify(ctx, a, false, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}

extern "C" zigz_status zigz_sumcheck_verify_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                            const uint64_t *eq_points, const size_t *ns, const unsigned *n_terms,
                                                            const unsigned *term_degrees, const uint8_t *term_tables,
                                                            const uint64_t *term_coeffs, const uint64_t *claimed_sums,
                                                            const uint64_t *rounds, const uint64_t *points, const uint64_t *table_evals,
                                                            const uint64_t *eq_evals, const uint64_t *final_evals, uint32_t flags,
                                                            uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                            size_t *n_rejected, size_t *bad_index) {
    ZIGZ_ENTER(ctx);
    if (!ctx) return ZIGZ_ERR_INVALID_ARGUMENT;
    const zc::VerifyArgs a{k, n_tables, (const void *const *)tables, eq_points, ns, n_terms, term_degrees, term_tables, term_coeffs,
                           claimed_sums, rounds, points, table_evals, eq_evals, final_evals, flags, n_rejected};
    CHK(host_value_checks(ctx, [&](bool *value) { return zc::check_verify_zerocheck_batch_host(a, bad_index, value); }));
    return verify(ctx, a, true, verdicts, expected_evals, oracle_evals, n_rejected, bad_index);
}
