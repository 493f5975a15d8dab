// Batched zero-check sumcheck with the eq factor in closed form: the round polynomials of
//   sum_{x in {0,1}^v} eq(tau, x) sum_{t < T} alpha_t prod_{j < d_t} pool[idx(t, j)](x),   d_t = 1..3,
// for k independent instances WITHOUT an eq table: the bind is MSB-first, round r binds index bit v - 1 - r, and
//   s_r(X) = P_r ((1 - tau_j) + (2 tau_j - 1) X) t_r(X),   t_r(X) = sum_{x < m/2} W_r[x] sum_t alpha_t prod_j (a_j[x] + X (b_j[x] - a_j[x])),
// with W_r = eq(tau_0 .. tau_{v-r-2}, .) (zerocheck_host.hpp).  The passes compute t_r, which has the degree of the constraint
// polynomial, and the host multiplies by the scalar and the linear factor.  They are sumcheck_sop.hip's passes -- the schedule,
// the chunking, the instantiation per pool size, the LDS parking, one loop per degree class, 16-byte non-temporal loads, the
// finish and tails launches themselves -- plus the weight:
//   k_zc_sums   round 0: reads the caller's tables and only sums;
//   k_zc_bind   every later round: binds every pool table with the previous challenge, stores it, sums the NEXT round's terms.
//
// The weight.  W_r[x] = lo[x & 1023] * hi_r[x >> 10]: lo = eq(tau_0 .. tau_9, .) is the same 1024 words (4 KiB, L2-resident) in
// every live round, hi_r = eq(tau_10 .. tau_{v-r-2}, .) has (pairs of round r) / 1024 words.  A live round has at least 1024
// pairs, so the split holds at every live length.  In one trip of a pass's loop the workgroup's 256 lanes hold 256 consecutive
// 16-byte vectors, i.e. the 1024 consecutive pairs 1024 g .. 1024 g + 1023 with g = (the workgroup's index in the instance) *
// ITERS + the trip: hi_r[g] is uniform over the trip, and lane l's four pairs have the low bits 4 l .. 4 l + 3 in EVERY trip.  So
// a lane loads lo[4 l .. 4 l + 3] as one 16-byte vector ONCE per workgroup and parks the four words in LDS next to the table words
// (holding them in registers across the table loads cost the fourth wave: 130 VGPRs instead of 126); a trip reads hi_r[g] as one
// scalar word, and a pair's weight is one Montgomery product of the two (both in Montgomery form, so W is too).  W then goes
// where alpha goes: the term's first factor is mont_mul(mont_mul(alpha_m, W_m), f0) -- canonical, no stray power of R -- one
// more Montgomery product per term and pair than the sop pass, and one per pair.
//
// Exact arithmetic.  With the weight folded into the first factor next to alpha, a term is still a plain product of d_t CANONICAL
// factors, so everything sumcheck_sop.hip states holds word for word: a lane's deferred lo / hi sums take at most 256 raw products
// before they are reduced, class 1 adds at most 8 canonical values per pair and coefficient unreduced, and the u64 sums over the
// workgroup and the instance cannot wrap (the static_asserts below restate them for this file's trip counts).  The power-of-1/R
// bookkeeping is unchanged (pd::sum_scale).  No atomics; every partial that is read is written by the same round's pass.
//
// The bind pass of an instance that is 2048 long sums for a round nobody reads (its next round is the host's); its descriptor
// names a valid one-word stage so that every load stays in bounds.
#include "sop_dev.hpp"

namespace zk {

namespace {

constexpr int ZC_TRIP_PAIRS = 4 * TPB;  // the pairs of one trip: 256 lanes x one 16-byte vector
static_assert(ZC_TRIP_PAIRS == 1 << ZC_LOG2_LO, "hi is uniform over a trip and a lane's lo words are the same in every trip");
static_assert(PRODUCT_CHUNK / 2 == SOP_SUM_ITERS * ZC_TRIP_PAIRS && PRODUCT_CHUNK / 4 == SOP_BIND_ITERS * ZC_TRIP_PAIRS,
              "a workgroup's pairs are whole trips: trip g of the instance is (workgroup) * ITERS + trip");
// The weighted first factor mont_mul(mont_mul(alpha_m, W_m), f0) is canonical like the sop pass's mont_mul(alpha_m, f0), so the
// counts of sumcheck_sop.hip apply unchanged:
// a lane's deferred sums: 2 products per term, pair and coefficient, 4 pairs per vector
static_assert(SOP_SUM_ITERS * 4 * 2 * SOP_MAX_TERMS <= 256 && SOP_BIND_ITERS * 4 * 2 * SOP_MAX_TERMS <= 256,
              "lo < 2^8 2^32, hi < 2^8 2^31: hi + monty_reduce(lo) < 2^40 < p 2^32");
// class 1: 8 canonical (weighted) values per pair and coefficient, unreduced; classes 2, 3: fewer lane values than pairs, each < 2^31
static_assert(3 + (PRODUCT_MAX_LOG2_N - 1) + 31 < 64, "a class coefficient's exact u64 sum: 2^3 * 2^29 * 2^31 < 2^64");
static_assert(P < (1u << 31), "a Montgomery product of two words below p is below p: W_m and alpha_m W_m stay canonical words");

struct ZcLds {
    SopLds s;
    uint32_t w[4 * TPB];  // [component][lane]: the lane's four words of lo, Montgomery form
};

// the lane's four lo words into LDS, once per workgroup (a lane reads back only what it wrote itself: no barrier)
__device__ __forceinline__ void zc_park_lo(const ZcWeights &w, ZcLds &l) {
    const zk_v4u e = *(const sop_gv4 *)((const sop_gchar *)w.lo + 16 * threadIdx.x);
    uint32_t *mine = l.w + threadIdx.x;
    mine[0 * TPB] = e.x;
    mine[1 * TPB] = e.y;
    mine[2 * TPB] = e.z;
    mine[3 * TPB] = e.w;
}
// the trip's hi word: uniform over the workgroup, scalar
__device__ __forceinline__ uint32_t zc_hi(const ZcWeights &w, uint32_t g) { return __builtin_amdgcn_readfirstlane(w.hi[g]); }

// sop_terms1 with the pair's weight next to alpha
template <int M, int C>
__device__ __forceinline__ void zc_terms1(const uint4 (&lo)[M], const uint4 (&hi)[M], uint32_t h_m, ZcLds &z, SopAcc &s) {
    SopLds &l = z.s;
    uint32_t *mine = l.f + threadIdx.x;
#pragma unroll
    for (int j = 0; j < M; j++) {
        mine[(2 * j) * TPB] = comp<C>(lo[j]);
        mine[(2 * j + 1) * TPB] = comp<C>(hi[j]);
    }
    const uint32_t w_m = mont_mul(z.w[C * TPB + threadIdx.x], h_m);  // W of this pair, Montgomery form
    const unsigned n_d1 = l.n_d1, n_d12 = l.n_d12, nterms = l.nterms;
    unsigned t = 0;
#pragma unroll 1
    for (; t < n_d1; t++) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(l.term[t].w), coef_m = __builtin_amdgcn_readfirstlane(l.term[t].coef_m);
        const SopFactor f0 = sop_factor(mine, w, 0);
        const uint32_t cw = mont_mul(coef_m, w_m);
        const uint32_t a[1] = {mont_mul(cw, f0.a)}, b[1] = {mont_mul(cw, f0.b)};
        pd_terms<1>(a, b, s.c1);
    }
#pragma unroll 1
    for (; t < n_d12; t++) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(l.term[t].w), coef_m = __builtin_amdgcn_readfirstlane(l.term[t].coef_m);
        const SopFactor f0 = sop_factor(mine, w, 0), f1 = sop_factor(mine, w, 1);
        const uint32_t cw = mont_mul(coef_m, w_m);
        const uint32_t a[2] = {mont_mul(cw, f0.a), f1.a}, b[2] = {mont_mul(cw, f0.b), f1.b};
        pd_terms<2>(a, b, s.c2);
    }
#pragma unroll 1
    for (; t < nterms; t++) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(l.term[t].w), coef_m = __builtin_amdgcn_readfirstlane(l.term[t].coef_m);
        const SopFactor f0 = sop_factor(mine, w, 0), f1 = sop_factor(mine, w, 1), f2 = sop_factor(mine, w, 2);
        const uint32_t cw = mont_mul(coef_m, w_m);
        const uint32_t a[3] = {mont_mul(cw, f0.a), f1.a, f2.a}, b[3] = {mont_mul(cw, f0.b), f1.b, f2.b};
        pd_terms<3>(a, b, s.c3);
    }
}

template <int M>
__device__ __forceinline__ void zc_terms4(const uint4 (&lo)[M], const uint4 (&hi)[M], uint32_t h_m, ZcLds &l, SopAcc &s) {
    zc_terms1<M, 0>(lo, hi, h_m, l, s);
    zc_terms1<M, 1>(lo, hi, h_m, l, s);
    zc_terms1<M, 2>(lo, hi, h_m, l, s);
    zc_terms1<M, 3>(lo, hi, h_m, l, s);
}

template <int M>
__device__ __forceinline__ void zc_sums(const SopTab &d, const ZcWeights &w, ZcLds &l, unsigned long long *__restrict__ part) {
    SopAcc s{};
    const uint32_t *in[M];
#pragma unroll
    for (int j = 0; j < M; j++) in[j] = d.in[j];
    const uint32_t hq = (uint32_t)(d.m / 8);  // 16-byte vectors per half; m >= 2048: hq / 256 >= 1 words of hi
    const uint32_t wg = blockIdx.x - d.first_wg;
    const uint32_t q0 = wg * (PRODUCT_CHUNK / 8) + threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < SOP_SUM_ITERS; it++) {
        const uint32_t q = q0 + (uint32_t)it * TPB;
        if (q < hq) {  // (q >> 8 == wg * SOP_SUM_ITERS + it < hq / 256)
            const uint32_t h_m = zc_hi(w, wg * SOP_SUM_ITERS + (uint32_t)it);
            uint4 a[M], b[M];
#pragma unroll
            for (int j = 0; j < M; j++) {
                a[j] = sop_load(in[j], 16 * q);
                b[j] = sop_load(in[j], 16 * (q + hq));
            }
            zc_terms4<M>(a, b, h_m, l, s);
        }
    }
    sop_store(s, part);
}

template <int M>
__device__ __forceinline__ void zc_bind(const SopTab &d, const ZcWeights &w, ZcLds &l, unsigned long long *__restrict__ part) {
    SopAcc s{};
    const uint32_t *in[M];
    uint32_t *out[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        in[j] = d.in[j];
        out[j] = d.out[j];
    }
    const uint32_t mq = (uint32_t)(d.m / 16);  // 16-byte vectors per quarter; m >= 4096: mq / 256 >= 1 words of hi (m == 2048: see above)
    const uint32_t wg = blockIdx.x - d.first_wg;
    const uint32_t q0 = wg * (PRODUCT_CHUNK / 16) + threadIdx.x;
    const uint32_t r_m = d.r_m;
#pragma unroll 1
    for (int it = 0; it < SOP_BIND_ITERS; it++) {
        const uint32_t q = q0 + (uint32_t)it * TPB;
        if (q < mq) {
            const uint32_t h_m = zc_hi(w, wg * SOP_BIND_ITERS + (uint32_t)it);
            uint4 lo[M], hi[M];
#pragma unroll
            for (int j = 0; j < M; j++) {  // (a table's four loads are in registers before its stores: out[j] may be in[j])
                const uint4 v0 = sop_load(in[j], 16 * q), v1 = sop_load(in[j], 16 * (q + mq)), v2 = sop_load(in[j], 16 * (q + 2 * mq)),
                            v3 = sop_load(in[j], 16 * (q + 3 * mq));
                lo[j] = pd_bind4(v0, v2, r_m);
                hi[j] = pd_bind4(v1, v3, r_m);
                sop_store16(out[j], 16 * q, lo[j]);
                sop_store16(out[j], 16 * (q + mq), hi[j]);
            }
            zc_terms4<M>(lo, hi, h_m, l, s);
        }
    }
    sop_store(s, part);
}

}  // namespace

__global__ __launch_bounds__(TPB) void k_zc_sums(const SopTab *__restrict__ tabs, const ZcWeights *__restrict__ ws, unsigned nt,
                                                 unsigned long long *__restrict__ part) {
    __shared__ ZcLds l;
    ZK_PRIO_SMALL();
    const unsigned x = find_first_wg(tabs, nt, blockIdx.x);
    const SopTab &d = tabs[x];
    const ZcWeights w = ws[x];
    zc_park_lo(w, l);
    sop_stage_terms(d, l.s);
    SOP_BY_POOL_SIZE(zc_sums, d, w, l, part)
}

__global__ __launch_bounds__(TPB) void k_zc_bind(const SopTab *__restrict__ tabs, const ZcWeights *__restrict__ ws, unsigned nt,
                                                 unsigned long long *__restrict__ part) {
    __shared__ ZcLds l;
    ZK_PRIO_SMALL();
    const unsigned x = find_first_wg(tabs, nt, blockIdx.x);
    const SopTab &d = tabs[x];
    const ZcWeights w = ws[x];
    zc_park_lo(w, l);
    sop_stage_terms(d, l.s);
    SOP_BY_POOL_SIZE(zc_bind, d, w, l, part)
}

void launch_zc_sums(const SopTab *d_tabs, const ZcWeights *d_w, unsigned nt, unsigned nwg, unsigned long long *d_part, hipStream_t s) {
    hipLaunchKernelGGL(k_zc_sums, dim3(nwg), dim3(TPB), 0, s, d_tabs, d_w, nt, d_part);
}
void launch_zc_bind(const SopTab *d_tabs, const ZcWeights *d_w, unsigned nt, unsigned nwg, unsigned long long *d_part, hipStream_t s) {
    hipLaunchKernelGGL(k_zc_bind, dim3(nwg), dim3(TPB), 0, s, d_tabs, d_w, nt, d_part);
}

}  // namespace zk
