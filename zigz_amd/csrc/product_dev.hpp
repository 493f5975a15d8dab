#pragma once
// Device helpers shared by the product sumcheck (sumcheck_product.hip) and the sum-of-products sumcheck (sumcheck_sop.hip): the
// coefficient terms of one index pair of d factors, added as raw 64-bit products with the reduction deferred, and the 16-byte bind.
// The arithmetic, its 1/R bookkeeping and its bounds are described at the head of sumcheck_product.hip.
#include "field.hpp"
#include "tree_dev.hpp"

namespace zk {

template <int D>
struct PdAcc {
    unsigned long long lo[D + 1], hi[D + 1];
};

__device__ __forceinline__ void pd_add(unsigned long long &lo, unsigned long long &hi, uint32_t x, uint32_t y) {
    const unsigned long long pr = (unsigned long long)x * y;
    lo += (uint32_t)pr;
    hi += pr >> 32;
}

// the terms of one index pair: a[j] = f_j at the low index, b[j] at the high one, canonical
template <int D>
__device__ __forceinline__ void pd_terms(const uint32_t (&a)[D], const uint32_t (&b)[D], PdAcc<D> &s) {
    uint32_t e[D];
#pragma unroll
    for (int j = 0; j < D; j++) e[j] = sub_mod(b[j], a[j]);
    if constexpr (D == 1) {
        s.lo[0] += a[0];
        s.lo[1] += e[0];
    } else if constexpr (D == 2) {
        pd_add(s.lo[0], s.hi[0], a[0], a[1]);
        pd_add(s.lo[1], s.hi[1], a[0], e[1]);
        pd_add(s.lo[1], s.hi[1], e[0], a[1]);
        pd_add(s.lo[2], s.hi[2], e[0], e[1]);
    } else {
        const uint32_t p = mont_mul(a[0], a[1]), q = mont_mul(e[0], e[1]);
        // a0 e1 + e0 a1 < 2 p^2 < p 2^32
        const uint32_t x = monty_reduce((unsigned long long)a[0] * e[1] + (unsigned long long)e[0] * a[1]);
        pd_add(s.lo[0], s.hi[0], p, a[2]);
        pd_add(s.lo[1], s.hi[1], p, e[2]);
        pd_add(s.lo[1], s.hi[1], x, a[2]);
        pd_add(s.lo[2], s.hi[2], x, e[2]);
        pd_add(s.lo[2], s.hi[2], q, a[2]);
        pd_add(s.lo[3], s.hi[3], q, e[2]);
    }
}

__device__ __forceinline__ uint4 pd_bind4(const uint4 &a, const uint4 &b, uint32_t r_m) {
    return make_uint4(bind1(a.x, b.x, r_m), bind1(a.y, b.y, r_m), bind1(a.z, b.z, r_m), bind1(a.w, b.w, r_m));
}

}  // namespace zk
