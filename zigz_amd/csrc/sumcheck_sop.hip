// Batched sum-of-products sumcheck: the round polynomials of
//   sum_{x in {0,1}^v}  sum_{t < T} alpha_t prod_{j < d_t} pool[idx(t, j)](x),   d_t = 1..3,
// for k independent instances with a pool of M <= 8 tables and T <= 8 terms each, one data pass per round.  The
// schedule, the chunking and the arithmetic are the product prover's (sumcheck_product.hip: MSB-first pairs, pd_terms, raw 64-bit
// products with the reduction deferred, exact u64 sums without atomics); what is new is that a term names its factors by pool
// index, so that a table shared by several terms -- the eq factor of a zero-check, above all -- is loaded, bound and stored once:
//   k_sop_sums    round 0: reads the caller's tables and only sums;
//   k_sop_bind    every later round: a lane loads T[q], T[q + m/4], T[q + m/2], T[q + 3m/4] of every pool table once, binds
//                 lo' and hi' with the previous challenge, stores them and multiplies out the NEXT round's terms of all terms
//                 from the bound values.  In place after the first bound round, as there; the caller's tables are never written.
//   k_sop_finish  one workgroup per instance: adds the partials, reduces mod p once, SOP_SUMS words into pinned memory; signals.
//   k_sop_tails   the pool tables of every instance once they are <= 1024 long into pinned memory.
//
// The term structure is run-time data, uniform over a workgroup, and a register array indexed by a run-time value would go to
// scratch.  So the tables' values are held in registers under compile-time indices only (the pass is instantiated per pool size
// M), and LDS is the lane's indexable register file: component by component of its 16-byte vectors (x, y, z, w: four index pairs)
// a lane parks the low and high word of every table at f[table][half][lane] -- word-strided, conflict-free, 16 KiB per
// workgroup -- and the term loop reads its factors back by pool index.  A lane reads only what it wrote itself, in program
// order, so no barrier is needed.  The terms (SopTerm: pool indices, alpha in Montgomery form; sorted by degree) are copied from the
// descriptor into LDS once per workgroup (the bind pass stores to global memory, after which the compiler could no longer read
// the descriptor with scalar loads) and read back at a uniform address, made scalar again with readfirstlane.
//
// Coefficient.  alpha_t goes into the term's first factor: a0' = alpha a0, b0' = alpha b0 (mont_mul with alpha in Montgomery
// form: canonical, no stray power of R), after which the term is a plain product of d_t canonical factors and pd_terms applies
// unchanged.  Terms of different degree carry different powers of 1/R, so a lane keeps one accumulator set per degree class
// (2 + 3 + 4 coefficient sums) and the host scales class d by R^d and adds the classes into c_0..c_D (sop_host.hpp).
//
// Exact arithmetic.  Per class coefficient a lane adds at most 2 raw products per term and index pair (pd_terms), T <= 8 terms,
// 4 pairs per vector and at most 4 vectors before it reduces: 256 products, lo < 2^40, hi < 2^39, hi + monty_reduce(lo) < 2^40
// < p 2^32.  Class 1 adds canonical values unreduced, at most 8 per pair and coefficient: over the 2^29 pairs of the largest
// table 2^3 2^29 2^31 = 2^63.  The reduced lane values of classes 2 and 3 are below 2^31 each and fewer than the pairs.  All of
// them are added in u64 (wave shuffle, four waves through LDS, one plain store per workgroup, the finish launch's sum).  Every
// partial that is read is written by the same round's pass: nothing is zeroed between rounds or calls.
#include "sop_dev.hpp"

namespace zk {

namespace {

template <int M, int C>
__device__ __forceinline__ void sop_terms1(const uint4 (&lo)[M], const uint4 (&hi)[M], SopLds &l, SopAcc &s) {
    uint32_t *mine = l.f + threadIdx.x;
#pragma unroll
    for (int j = 0; j < M; j++) {
        mine[(2 * j) * TPB] = comp<C>(lo[j]);
        mine[(2 * j + 1) * TPB] = comp<C>(hi[j]);
    }
    // One loop per degree class, so that a loop carries only its own class's sums.  w and coef_m are uniform: scalar again.
    const unsigned n_d1 = l.n_d1, n_d12 = l.n_d12, nterms = l.nterms;
    unsigned t = 0;
#pragma unroll 1
    for (; t < n_d1; t++) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(l.term[t].w), coef_m = __builtin_amdgcn_readfirstlane(l.term[t].coef_m);
        const SopFactor f0 = sop_factor(mine, w, 0);
        const uint32_t a[1] = {mont_mul(coef_m, f0.a)}, b[1] = {mont_mul(coef_m, f0.b)};
        pd_terms<1>(a, b, s.c1);
    }
#pragma unroll 1
    for (; t < n_d12; t++) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(l.term[t].w), coef_m = __builtin_amdgcn_readfirstlane(l.term[t].coef_m);
        const SopFactor f0 = sop_factor(mine, w, 0), f1 = sop_factor(mine, w, 1);
        const uint32_t a[2] = {mont_mul(coef_m, f0.a), f1.a}, b[2] = {mont_mul(coef_m, f0.b), f1.b};
        pd_terms<2>(a, b, s.c2);
    }
#pragma unroll 1
    for (; t < nterms; t++) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(l.term[t].w), coef_m = __builtin_amdgcn_readfirstlane(l.term[t].coef_m);
        const SopFactor f0 = sop_factor(mine, w, 0), f1 = sop_factor(mine, w, 1), f2 = sop_factor(mine, w, 2);
        const uint32_t a[3] = {mont_mul(coef_m, f0.a), f1.a, f2.a}, b[3] = {mont_mul(coef_m, f0.b), f1.b, f2.b};
        pd_terms<3>(a, b, s.c3);
    }
}

template <int M>
__device__ __forceinline__ void sop_terms4(const uint4 (&lo)[M], const uint4 (&hi)[M], SopLds &l, SopAcc &s) {
    sop_terms1<M, 0>(lo, hi, l, s);
    sop_terms1<M, 1>(lo, hi, l, s);
    sop_terms1<M, 2>(lo, hi, l, s);
    sop_terms1<M, 3>(lo, hi, l, s);
}

template <int M>
__device__ __forceinline__ void sop_sums(const SopTab &d, SopLds &l, unsigned long long *__restrict__ part) {
    SopAcc s{};
    const uint32_t *in[M];
#pragma unroll
    for (int j = 0; j < M; j++) in[j] = d.in[j];
    const uint32_t hq = (uint32_t)(d.m / 8);  // 16-byte vectors per half; m >= 2048
    const uint32_t q0 = (blockIdx.x - d.first_wg) * (PRODUCT_CHUNK / 8) + threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < SOP_SUM_ITERS; it++) {
        const uint32_t q = q0 + (uint32_t)it * TPB;
        if (q < hq) {
            uint4 a[M], b[M];
#pragma unroll
            for (int j = 0; j < M; j++) {
                a[j] = sop_load(in[j], 16 * q);
                b[j] = sop_load(in[j], 16 * (q + hq));
            }
            sop_terms4<M>(a, b, l, s);
        }
    }
    sop_store(s, part);
}

template <int M>
__device__ __forceinline__ void sop_bind(const SopTab &d, SopLds &l, unsigned long long *__restrict__ part) {
    SopAcc s{};
    const uint32_t *in[M];
    uint32_t *out[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        in[j] = d.in[j];
        out[j] = d.out[j];
    }
    const uint32_t mq = (uint32_t)(d.m / 16);  // 16-byte vectors per quarter; m >= 2048
    const uint32_t q0 = (blockIdx.x - d.first_wg) * (PRODUCT_CHUNK / 16) + threadIdx.x;
    const uint32_t r_m = d.r_m;
#pragma unroll 1
    for (int it = 0; it < SOP_BIND_ITERS; it++) {
        const uint32_t q = q0 + (uint32_t)it * TPB;
        if (q < mq) {
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
            sop_terms4<M>(lo, hi, l, s);
        }
    }
    sop_store(s, part);
}

}  // namespace

__global__ __launch_bounds__(TPB) void k_sop_sums(const SopTab *__restrict__ tabs, unsigned nt, unsigned long long *__restrict__ part) {
    __shared__ SopLds l;
    ZK_PRIO_SMALL();
    const SopTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    sop_stage_terms(d, l);
    SOP_BY_POOL_SIZE(sop_sums, d, l, part)
}

__global__ __launch_bounds__(TPB) void k_sop_bind(const SopTab *__restrict__ tabs, unsigned nt, unsigned long long *__restrict__ part) {
    __shared__ SopLds l;
    ZK_PRIO_SMALL();
    const SopTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    sop_stage_terms(d, l);
    SOP_BY_POOL_SIZE(sop_bind, d, l, part)
}

// One workgroup per instance: for every class coefficient the partial sums of the instance's workgroups (SOP_SUMS words per
// workgroup, consecutive) added up, reduced mod p once and written at the instance's result words in pinned memory.
__global__ __launch_bounds__(TPB) void k_sop_finish(const SopTab *__restrict__ tabs, const unsigned long long *__restrict__ part,
                                                    uint64_t *out, DoneFlag done) {
    __shared__ unsigned long long s_sum[SOP_SUMS][TPB / 64];
    const SopTab &d = tabs[blockIdx.x];
    const size_t cnt = (size_t)((d.m + PRODUCT_CHUNK - 1) / PRODUCT_CHUNK);
    const unsigned long long *p = part + (size_t)d.first_wg * SOP_SUMS;
    for (unsigned c = 0; c < SOP_SUMS; c++) {
        unsigned long long sum = 0;
        for (size_t j = threadIdx.x; j < cnt; j += TPB) sum += p[j * SOP_SUMS + c];
        sum = wave_sum(sum);
        if ((threadIdx.x & 63) == 0) s_sum[c][threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    if (threadIdx.x < SOP_SUMS)
        out[(size_t)d.slot * SOP_SUMS + threadIdx.x] =
            (s_sum[threadIdx.x][0] + s_sum[threadIdx.x][1] + s_sum[threadIdx.x][2] + s_sum[threadIdx.x][3]) % (unsigned long long)P;
    signal_done_block(done, gridDim.x);  // (TPB threads: several waves; no thread returns early)
}

// One workgroup per instance: its current pool tables (m <= 1024 values each) into pinned memory, u32, one behind the other.
__global__ __launch_bounds__(TPB) void k_sop_tails(const SopTab *__restrict__ tabs, uint32_t *h_dst, DoneFlag done) {
    const SopTab &d = tabs[blockIdx.x];
    const size_t m = (size_t)d.m;
    for (unsigned j = 0; j < d.n_tables; j++)
        for (size_t i = threadIdx.x; i < m; i += TPB) h_dst[d.tail_off + j * m + i] = d.in[j][i];
    signal_done_block(done, gridDim.x);
}

void launch_sop_sums(const SopTab *d_tabs, unsigned nt, unsigned nwg, unsigned long long *d_part, hipStream_t s) {
    hipLaunchKernelGGL(k_sop_sums, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, d_part);
}
void launch_sop_bind(const SopTab *d_tabs, unsigned nt, unsigned nwg, unsigned long long *d_part, hipStream_t s) {
    hipLaunchKernelGGL(k_sop_bind, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, d_part);
}
void launch_sop_finish(const SopTab *d_tabs, unsigned nt, const unsigned long long *d_part, uint64_t *out, hipStream_t s, DoneFlag done) {
    hipLaunchKernelGGL(k_sop_finish, dim3(nt), dim3(TPB), 0, s, d_tabs, d_part, out, done);
}
void launch_sop_tails(const SopTab *d_tabs, unsigned nt, uint32_t *h_dst, hipStream_t s, DoneFlag done) {
    hipLaunchKernelGGL(k_sop_tails, dim3(nt), dim3(TPB), 0, s, d_tabs, h_dst, done);
}

}  // namespace zk
