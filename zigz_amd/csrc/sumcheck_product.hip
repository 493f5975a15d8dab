// Batched product sumcheck: the round polynomials of  sum_{x in {0,1}^v} prod_{j<d} f_j(x),  d = 1..3, for k independent
// instances of different lengths and degrees, one data pass per round and instance-independent launch counts.
//
// Round polynomial.  With a_j = f_j[i], b_j = f_j[i + m/2] (i < m/2; MSB-first, as partialEval binds) and e_j = b_j - a_j,
//   g(t) = sum_i prod_j (a_j + t e_j) = c_0 + c_1 t + .. + c_d t^d,
//   d = 1:  c = (a, e)        d = 2:  c = (a0 a1,  a0 e1 + e0 a1,  e0 e1)
//   d = 3:  with P = a0 a1, X = a0 e1 + e0 a1, Q = e0 e1:  c = (P a2,  P e2 + X a2,  X e2 + Q a2,  Q e2).
// The radix schedule of the linear prover does not carry over (several rounds follow from block sums only because the sum is
// linear in the table), so every round reads the tables once:
//   k_product_sums   round 0: reads the caller's tables and only sums;
//   k_product_bind   every later round: a lane loads T[q], T[q + m/4], T[q + m/2], T[q + 3m/4] of every factor (q < m/4), binds
//                    lo' = bind(T[q], T[q + m/2]) and hi' = bind(T[q + m/4], T[q + 3m/4]) with the previous challenge, stores them
//                    at q and q + m/4 of the bound table and multiplies out the NEXT round's terms from (lo', hi').  A lane
//                    writes only words that it alone reads (and has loaded before it stores), so once the tables are the
//                    call's own copy -- after the first bound round, which reads the caller's tables and writes n/2 words per
//                    factor into the workspace -- the pass runs in place.  The caller's tables are never written, and the
//                    same table may serve as several factors: every factor has a bound copy of its own.
//   k_product_finish one workgroup per instance: adds the instance's partial sums, reduces mod p ONCE and writes the d + 1
//                    sums into pinned memory; signals the host (signal_done_block).
//   k_product_tails  the tables of every instance once they are <= 1024 long into pinned memory: the host runs the last rounds.
// The layout is mle_batch.hip's: a table of per-instance descriptors (ProductTab, kernels.hpp), find_first_wg, streaming
// 16-byte loads, one workgroup per chunk of PRODUCT_CHUNK elements.
//
// Inner product.  Tables hold canonical values, so a product of two of them through the Montgomery reduction carries a factor
// 1/R; instead of repairing that per element the kernels let it ride: 32-bit multiplies issue at under half rate on gfx950
// (k_radix_fold), so the terms are added as raw 64-bit products, low and high halves apart (k_mle_batch_eval's deferred
// reduction), and a lane reduces twice at the end:  monty_reduce(hi + monty_reduce(lo)) = (sum of the products) / R^2, canonical.
// For d = 3 the inner factors P, X, Q are reduced once (/R) before the outer multiply.  So a published sum is the coefficient
// times R^-d (d >= 2) or the coefficient itself (d = 1); the host multiplies by R^d mod p (product_host.hpp: coefficients()).
//
// Exact arithmetic: every term a workgroup adds is a canonical value below p; a coefficient has at most three product terms
// per index pair (here at most two: X is reduced as one), a lane adds its pairs' terms before it reduces, and the per-lane
// values -- fewer than 3 * 2^29 of them, each below 2^31 -- are added in u64: a shuffle sum per wave, the four waves through LDS,
// ONE plain store per workgroup and coefficient into a partial array indexed by the workgroup's number (no atomics), and the
// finish launch's sum over the instance's workgroups.  Every partial that is read is written by the same round's pass, so
// nothing has to be zeroed between rounds or calls.
#include "kernels.hpp"

#include "product_dev.hpp"  // PdAcc, pd_add, pd_terms, pd_bind4 (with field.hpp, tree_dev.hpp)

namespace zk {

namespace {

constexpr int PD_SUM_ITERS = PRODUCT_CHUNK / (8 * TPB);    // round 0: a lane's 16-byte index-pair vectors (i, i + m/2)
constexpr int PD_BIND_ITERS = PRODUCT_CHUNK / (16 * TPB);  // bind pass: a lane's 16-byte quadruples (q, q + m/4, q + m/2, q + 3m/4)
static_assert(PD_SUM_ITERS == 4 && PD_BIND_ITERS == 2, "a workgroup owns PRODUCT_CHUNK elements of the current table");
static_assert(TPB == 256, "four wave sums per workgroup and coefficient");
// 3 terms below p < 2^31 per index pair, 2^(log2 n - 1) pairs
static_assert(2 + (PRODUCT_MAX_LOG2_N - 1) + 31 < 64, "a coefficient's exact u64 sum: 3 * 2^29 * 2^31 < 2^64");
// a lane's deferred sums: at most 2 products per pair and coefficient, 4 pairs per vector -> lo < 2^5 2^32, hi < 2^5 2^31
static_assert(PD_SUM_ITERS * 4 * 2 <= 32 && PD_BIND_ITERS * 4 * 2 <= 32, "hi + monty_reduce(lo) < 2^37 < p 2^32");

template <int D>
__device__ __forceinline__ void pd_terms4(const uint4 (&a)[D], const uint4 (&b)[D], PdAcc<D> &s) {
    uint32_t x[D], y[D];
#pragma unroll
    for (int j = 0; j < D; j++) { x[j] = a[j].x; y[j] = b[j].x; }
    pd_terms<D>(x, y, s);
#pragma unroll
    for (int j = 0; j < D; j++) { x[j] = a[j].y; y[j] = b[j].y; }
    pd_terms<D>(x, y, s);
#pragma unroll
    for (int j = 0; j < D; j++) { x[j] = a[j].z; y[j] = b[j].z; }
    pd_terms<D>(x, y, s);
#pragma unroll
    for (int j = 0; j < D; j++) { x[j] = a[j].w; y[j] = b[j].w; }
    pd_terms<D>(x, y, s);
}

// the lane's sums -> canonical values, added over the workgroup, one store per coefficient at part[PRODUCT_SUMS wg + c]
template <int D>
__device__ __forceinline__ void pd_store(const PdAcc<D> &s, unsigned long long *__restrict__ part) {
    __shared__ unsigned long long s_sum[PRODUCT_SUMS][TPB / 64];
    const unsigned t = threadIdx.x;
#pragma unroll
    for (int c = 0; c <= D; c++) {
        unsigned long long term = D == 1 ? s.lo[c] : (unsigned long long)monty_reduce(s.hi[c] + monty_reduce(s.lo[c]));
        term = wave_sum(term);
        if ((t & 63) == 0) s_sum[c][t >> 6] = term;
    }
    __syncthreads();
    if (t <= (unsigned)D) part[(size_t)blockIdx.x * PRODUCT_SUMS + t] = s_sum[t][0] + s_sum[t][1] + s_sum[t][2] + s_sum[t][3];
}

template <int D>
__device__ __forceinline__ void pd_sums(const ProductTab &d, unsigned long long *__restrict__ part) {
    PdAcc<D> s{};
    const size_t hq = (size_t)(d.m / 8);  // 16-byte vectors per half; m >= 2048
    const size_t q0 = (size_t)(blockIdx.x - d.first_wg) * (PRODUCT_CHUNK / 8) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < PD_SUM_ITERS; it++) {
        const size_t q = q0 + (size_t)it * TPB;
        if (q < hq) {
            uint4 a[D], b[D];
#pragma unroll
            for (int j = 0; j < D; j++) {
                const uint4 *p = reinterpret_cast<const uint4 *>(d.in[j]);
                a[j] = stream_load(p + q);
                b[j] = stream_load(p + q + hq);
            }
            pd_terms4<D>(a, b, s);
        }
    }
    pd_store<D>(s, part);
}

template <int D>
__device__ __forceinline__ void pd_bind(const ProductTab &d, unsigned long long *__restrict__ part) {
    PdAcc<D> s{};
    const size_t mq = (size_t)(d.m / 16);  // 16-byte vectors per quarter; m >= 2048
    const size_t q0 = (size_t)(blockIdx.x - d.first_wg) * (PRODUCT_CHUNK / 16) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < PD_BIND_ITERS; it++) {
        const size_t q = q0 + (size_t)it * TPB;
        if (q < mq) {
            uint4 v[D][4];
#pragma unroll
            for (int j = 0; j < D; j++) {
                const uint4 *p = reinterpret_cast<const uint4 *>(d.in[j]);
#pragma unroll
                for (int h = 0; h < 4; h++) v[j][h] = stream_load(p + q + (size_t)h * mq);
            }
            uint4 lo[D], hi[D];
#pragma unroll
            for (int j = 0; j < D; j++) {  // (all of the lane's loads are in registers: out[j] may be in[j])
                lo[j] = pd_bind4(v[j][0], v[j][2], d.r_m);
                hi[j] = pd_bind4(v[j][1], v[j][3], d.r_m);
                uint4 *o = reinterpret_cast<uint4 *>(d.out[j]);
                o[q] = lo[j];
                o[q + mq] = hi[j];
            }
            pd_terms4<D>(lo, hi, s);
        }
    }
    pd_store<D>(s, part);
}

}  // namespace

__global__ __launch_bounds__(TPB) void k_product_sums(const ProductTab *__restrict__ tabs, unsigned nt,
                                                      unsigned long long *__restrict__ part) {
    ZK_PRIO_SMALL();
    const ProductTab d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    if (d.d == 1) pd_sums<1>(d, part);  // uniform over the workgroup
    else if (d.d == 2) pd_sums<2>(d, part);
    else pd_sums<3>(d, part);
}

__global__ __launch_bounds__(TPB) void k_product_bind(const ProductTab *__restrict__ tabs, unsigned nt,
                                                      unsigned long long *__restrict__ part) {
    ZK_PRIO_SMALL();
    const ProductTab d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    if (d.d == 1) pd_bind<1>(d, part);
    else if (d.d == 2) pd_bind<2>(d, part);
    else pd_bind<3>(d, part);
}

// One workgroup per instance: for every coefficient the partial sums of the instance's workgroups (PRODUCT_SUMS words per
// workgroup, consecutive) added up, reduced mod p once and written at the instance's result words in pinned memory.
__global__ __launch_bounds__(TPB) void k_product_finish(const ProductTab *__restrict__ tabs, const unsigned long long *__restrict__ part,
                                                        uint64_t *out, DoneFlag done) {
    __shared__ unsigned long long s_sum[PRODUCT_SUMS][TPB / 64];
    const ProductTab &d = tabs[blockIdx.x];
    const size_t cnt = (size_t)((d.m + PRODUCT_CHUNK - 1) / PRODUCT_CHUNK);
    const unsigned long long *p = part + (size_t)d.first_wg * PRODUCT_SUMS;
    const unsigned nc = d.d + 1;
    for (unsigned c = 0; c < nc; c++) {  // uniform
        unsigned long long sum = 0;
        for (size_t j = threadIdx.x; j < cnt; j += TPB) sum += p[j * PRODUCT_SUMS + c];
        sum = wave_sum(sum);
        if ((threadIdx.x & 63) == 0) s_sum[c][threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    if (threadIdx.x < nc)
        out[(size_t)d.slot * PRODUCT_SUMS + threadIdx.x] =
            (s_sum[threadIdx.x][0] + s_sum[threadIdx.x][1] + s_sum[threadIdx.x][2] + s_sum[threadIdx.x][3]) % (unsigned long long)P;
    signal_done_block(done, gridDim.x);  // (TPB threads: several waves; no thread returns early)
}

// One workgroup per instance: its d current tables (m <= 1024 values each) into pinned memory, u32, one behind the other.
__global__ __launch_bounds__(TPB) void k_product_tails(const ProductTab *__restrict__ tabs, uint32_t *h_dst, DoneFlag done) {
    const ProductTab &d = tabs[blockIdx.x];
    const size_t m = (size_t)d.m;
    for (unsigned j = 0; j < d.d; j++)
        for (size_t i = threadIdx.x; i < m; i += TPB) h_dst[d.tail_off + j * m + i] = d.in[j][i];
    signal_done_block(done, gridDim.x);
}

void launch_product_sums(const ProductTab *d_tabs, unsigned nt, unsigned nwg, unsigned long long *d_part, hipStream_t s) {
    hipLaunchKernelGGL(k_product_sums, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, d_part);
}
void launch_product_bind(const ProductTab *d_tabs, unsigned nt, unsigned nwg, unsigned long long *d_part, hipStream_t s) {
    hipLaunchKernelGGL(k_product_bind, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, d_part);
}
void launch_product_finish(const ProductTab *d_tabs, unsigned nt, const unsigned long long *d_part, uint64_t *out, hipStream_t s,
                           DoneFlag done) {
    hipLaunchKernelGGL(k_product_finish, dim3(nt), dim3(TPB), 0, s, d_tabs, d_part, out, done);
}
void launch_product_tails(const ProductTab *d_tabs, unsigned nt, uint32_t *h_dst, hipStream_t s, DoneFlag done) {
    hipLaunchKernelGGL(k_product_tails, dim3(nt), dim3(TPB), 0, s, d_tabs, h_dst, done);
}

}  // namespace zk
