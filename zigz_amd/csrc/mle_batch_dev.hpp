// Device-side set-up shared by the two kernels that walk a table in chunks of MLE_BATCH_CHUNK elements and need the eq weight
// prod_v f_v[bit v of i] of every element i: k_mle_batch_eval (mle_batch.hip), which multiplies the weights into a table and adds
// them up, and k_eq_batch_expand (eq_batch.hip), which writes them out.
//
// The chunk layout i = base + 4 (256 j + thread) + c splits the index bits into
//   bits  0-1  c       and bits 10-12  j : 32 workgroup-uniform weights U[j][c], built once per workgroup in LDS
//   bits  2-9  thread                    : two 16-entry tables A (bits 2-5), B (bits 6-9) in LDS, one product per lane
//   bits 13+   workgroup                 : one uniform factor H (a product over the lanes of one wave)
// A variable past the table's own (a table smaller than a chunk) has the factor pair (1, 0): every element that does not exist
// gets weight 0.
#pragma once
#include "kernels.hpp"

#include "field.hpp"
#include "tree_dev.hpp"

namespace zk {

constexpr int ME_LOADS = MLE_BATCH_CHUNK / (4 * TPB);  // 16-byte accesses per lane
constexpr unsigned ME_LANE_BIT = 2, ME_LOOP_BIT = 10, ME_HI_BIT = 13;  // first index bit of the thread, the access, the workgroup
static_assert(ME_LOADS == 8 && MLE_BATCH_CHUNK == 1u << ME_HI_BIT, "index bits: 2 component, 8 thread, 3 load, the rest workgroup");
static_assert(TPB == 256, "A and B cover the thread's 8 index bits, wave 1 the high variables, four wave sums per workgroup");
static_assert(ME_HI_BIT + 64 > MLE_BATCH_MAX_LOG2_N, "one wave holds a factor per high variable");

// prod_{i < cnt} f_{v0 + i}[bit i of bits], Montgomery form; a variable the table does not have contributes (1, 0)
__device__ __forceinline__ uint32_t me_eq(const uint32_t *__restrict__ f, unsigned nv, unsigned v0, unsigned cnt, unsigned bits) {
    uint32_t w = R_MOD_P;
    for (unsigned i = 0; i < cnt; i++) {
        const unsigned v = v0 + i, b = (bits >> i) & 1;
        w = mont_mul(w, v < nv ? f[2 * v + b] : (b ? 0u : R_MOD_P));
    }
    return w;
}

// The workgroup's weights for the chunk at `base` of a table of nv variables with the factor pairs f (kernels.hpp: MleBatchTab
// f_off), into LDS: s_u[4 j + c] = U[j][c] (32 words), s_a, s_b (16 words each) in Montgomery form, and *s_hi = H hi_scale / R --
// what the caller needs H to carry (k_mle_batch_eval: R^2, giving H R^2; k_eq_batch_expand: 1, giving H itself, canonical).
// Ends with the barrier that makes them visible.  Every thread of the workgroup must call it.
__device__ __forceinline__ void me_chunk_weights(const uint32_t *__restrict__ f, unsigned nv, size_t base, unsigned t, uint32_t hi_scale,
                                                 uint32_t *s_u, uint32_t *s_a, uint32_t *s_b, uint32_t *s_hi) {
    if (t < 32) {
        s_u[t] = mont_mul(me_eq(f, nv, 0, ME_LANE_BIT, t & 3), me_eq(f, nv, ME_LOOP_BIT, ME_HI_BIT - ME_LOOP_BIT, t >> 2));
    } else if (t < 48) {
        s_a[t - 32] = me_eq(f, nv, ME_LANE_BIT, 4, t - 32);
    } else if (t < 64) {
        s_b[t - 48] = me_eq(f, nv, ME_LANE_BIT + 4, 4, t - 48);
    } else if (t < 128) {  // wave 1: H, the factors of the workgroup's own index bits multiplied across the lanes
        const unsigned v = ME_HI_BIT + (t - 64);
        uint32_t w = v < nv ? f[2 * v + (unsigned)((base >> v) & 1)] : R_MOD_P;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) w = mont_mul(w, __shfl_down(w, off, 64));
        if (t == 64) *s_hi = mont_mul(w, hi_scale);
    }
    __syncthreads();
}

}  // namespace zk
