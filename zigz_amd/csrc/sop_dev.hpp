#pragma once
// Device helpers shared by the sum-of-products sumcheck (sumcheck_sop.hip) and the closed-form zero-check (sumcheck_zerocheck.hip):
// the chunking constants and the exactness bounds of a pass, the 16-byte non-temporal accesses, the LDS parking of a lane's table
// words, the staging of an instance's terms, the workgroup sum of the class coefficients and the instantiation per pool size.  The
// arithmetic and its bounds are described at the head of sumcheck_sop.hip.
#include "kernels.hpp"

#include "product_dev.hpp"

namespace zk {

constexpr int SOP_SUM_ITERS = PRODUCT_CHUNK / (8 * TPB);    // round 0: a lane's 16-byte index-pair vectors (i, i + m/2)
constexpr int SOP_BIND_ITERS = PRODUCT_CHUNK / (16 * TPB);  // bind pass: a lane's 16-byte quadruples
static_assert(SOP_SUM_ITERS == 4 && SOP_BIND_ITERS == 2, "a workgroup owns PRODUCT_CHUNK elements of the current table");
static_assert(TPB == 256, "four wave sums per workgroup and coefficient");
static_assert(SOP_MAX_TERMS == 8 && PRODUCT_MAX_DEGREE == 3 && SOP_SUMS == 9, "the bounds below are for 8 terms of degree <= 3");
// a lane's deferred sums: 2 products per term, pair and coefficient, 4 pairs per vector
static_assert(SOP_SUM_ITERS * 4 * 2 * SOP_MAX_TERMS <= 256 && SOP_BIND_ITERS * 4 * 2 * SOP_MAX_TERMS <= 256,
              "lo < 2^8 2^32, hi < 2^8 2^31: hi + monty_reduce(lo) < 2^40 < p 2^32");
// class 1: 8 canonical values per pair and coefficient, unreduced; classes 2, 3: fewer lane values than pairs, each below 2^31
static_assert(3 + (PRODUCT_MAX_LOG2_N - 1) + 31 < 64, "a class coefficient's exact u64 sum: 2^3 * 2^29 * 2^31 < 2^64");

struct SopAcc {
    PdAcc<1> c1;
    PdAcc<2> c2;
    PdAcc<3> c3;
};

// The tables' addresses come out of the descriptor, so the compiler takes them for generic pointers and would use flat
// accesses, which count against the LDS counter as well: say that they are global memory.
// A table is at most 2^30 words, so a byte offset into it fits 32 bits: uniform base (scalar registers) + one offset register per
// access instead of a 64-bit address each.
typedef zk_v4u __attribute__((address_space(1))) sop_gv4;
typedef char __attribute__((address_space(1))) sop_gchar;
static_assert(PRODUCT_MAX_LOG2_N + 2 <= 32, "byte offsets into a table fit 32 bits");
__device__ __forceinline__ uint4 sop_load(const uint32_t *base, uint32_t byte_off) {  // global_load_dwordx4 ... nt
    const zk_v4u v = __builtin_nontemporal_load((const sop_gv4 *)((const sop_gchar *)base + byte_off));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void sop_store16(uint32_t *base, uint32_t byte_off, const uint4 &v) {  // global_store_dwordx4
    *(sop_gv4 *)((sop_gchar *)base + byte_off) = zk_v4u{v.x, v.y, v.z, v.w};
}

template <int C>
__device__ __forceinline__ uint32_t comp(const uint4 &v) {
    return C == 0 ? v.x : C == 1 ? v.y : C == 2 ? v.z : v.w;
}

// One component of the lane's vectors: parks (lo[j], hi[j]) of the M tables in LDS and adds the terms of every term of the
// instance for that index pair.  SopLds::f is [SOP_MAX_TABLES][2][TPB]; the lane touches column threadIdx.x only.
struct SopLds {
    uint32_t f[SOP_MAX_TABLES * 2 * TPB];
    SopTerm term[SOP_MAX_TERMS];
    unsigned n_d1, n_d12, nterms;  // the terms are sorted by degree: [0, n_d1) linear, [n_d1, n_d12) quadratic, the rest cubic
};
struct SopFactor {
    uint32_t a, b;
};
// term t's factor j of this lane: the low and the high word of the pool table the term names
__device__ __forceinline__ SopFactor sop_factor(const uint32_t *mine, uint32_t w, int j) {
    const unsigned i = (w >> (8 + 8 * j)) & 0xFF;
    return SopFactor{mine[(2 * i) * TPB], mine[(2 * i + 1) * TPB]};
}

// the instance's terms into LDS, before any of the pass's stores
__device__ __forceinline__ void sop_stage_terms(const SopTab &d, SopLds &l) {
    if (threadIdx.x < SOP_MAX_TERMS) l.term[threadIdx.x] = d.term[threadIdx.x];
    if (threadIdx.x == 0) {
        l.n_d1 = d.n_d1;
        l.n_d12 = d.n_d1 + d.n_d2;
        l.nterms = d.n_terms;
    }
    __syncthreads();
}

// the lane's sums -> canonical values (class 1: the plain sums), added over the workgroup, one store per class coefficient at
// part[SOP_SUMS wg + c]
__device__ __forceinline__ void sop_store(const SopAcc &s, unsigned long long *__restrict__ part) {
    __shared__ unsigned long long s_sum[SOP_SUMS][TPB / 64];
    const unsigned t = threadIdx.x;
    unsigned long long term[SOP_SUMS];
    term[0] = s.c1.lo[0];
    term[1] = s.c1.lo[1];
#pragma unroll
    for (int c = 0; c < 3; c++) term[SOP_CLASS_AT[1] + c] = monty_reduce(s.c2.hi[c] + monty_reduce(s.c2.lo[c]));
#pragma unroll
    for (int c = 0; c < 4; c++) term[SOP_CLASS_AT[2] + c] = monty_reduce(s.c3.hi[c] + monty_reduce(s.c3.lo[c]));
#pragma unroll
    for (int c = 0; c < (int)SOP_SUMS; c++) {
        const unsigned long long w = wave_sum(term[c]);
        if ((t & 63) == 0) s_sum[c][t >> 6] = w;
    }
    __syncthreads();
    if (t < SOP_SUMS) part[(size_t)blockIdx.x * SOP_SUMS + t] = s_sum[t][0] + s_sum[t][1] + s_sum[t][2] + s_sum[t][3];
}

}  // namespace zk

#define SOP_BY_POOL_SIZE(fn, d, ...)                   \
    switch ((d).n_tables) { /* uniform over the workgroup */ \
        case 1: fn<1>(d, __VA_ARGS__); break;          \
        case 2: fn<2>(d, __VA_ARGS__); break;          \
        case 3: fn<3>(d, __VA_ARGS__); break;          \
        case 4: fn<4>(d, __VA_ARGS__); break;          \
        case 5: fn<5>(d, __VA_ARGS__); break;          \
        case 6: fn<6>(d, __VA_ARGS__); break;          \
        case 7: fn<7>(d, __VA_ARGS__); break;          \
        default: fn<8>(d, __VA_ARGS__); break;         \
    }
