// Batched eq tables: E[x] = prod_v f_v[bit v of x], f_v = (1 - tau_v, tau_v), for k independent (length, tau) pairs in ONE launch
// (zigz_[dev_]eq_table_batch).  E is the table of weights Multilinear.eval (multilinear.zig:110-144) multiplies
// into a table, so sum_x E[x] T[x] = eval(T, tau) exactly; a zero-check proves sum_x E[x] C(x) = 0 with E as the first factor of
// a product sumcheck (sumcheck_product.hip).
//
// The layout is k_mle_batch_eval's (mle_batch.hip; the set-up is the same device function, mle_batch_dev.hpp): a table of
// per-table descriptors (EqBatchTab, kernels.hpp), find_first_wg, one workgroup per chunk of MLE_BATCH_CHUNK (8192) consecutive
// words, the chunk's weights U (32, workgroup-uniform), A, B (16 each, by thread) and H (the workgroup's own index bits) built
// once in LDS.  H leaves the set-up in canonical form, so a lane's weight w = A B H is canonical and word 4 (256 j + t) + c is
// the ONE Montgomery product U[j][c] w per element -- canonical out, no conversion pass.
//
// Stores: 8 x 16 bytes per lane, lane t of store j at quad q0 + 256 j + t -- a wave writes 1 KiB contiguously per instruction.
// Plain stores, not non-temporal ones: either kind leaves the chip's L2 once per pass, and the table's only reader is the launch
// queued right behind (round 0 of the product prover, an eval), which finds a table of up to a few MiB still in the caches
// when the stores did not ask for it to be dropped.  A table shorter than a chunk is one partial workgroup whose stores
// are guarded by the table's length (the words that do not exist have weight 0 and are not written); a table of 1 or 2 words
// has no 16 bytes to store and is written word by word by lane 0.  Nothing is read but the descriptors and the factors.
#include "mle_batch_dev.hpp"

namespace zk {

typedef __attribute__((address_space(1))) zk_v4u eq_v4u_global;

__global__ __launch_bounds__(TPB) void k_eq_batch_expand(const EqBatchTab *__restrict__ tabs, unsigned nt,
                                                         const uint32_t *__restrict__ factors) {
    ZK_PRIO_SMALL();
    __shared__ __align__(16) uint32_t s_u[4 * ME_LOADS];
    __shared__ uint32_t s_a[16], s_b[16], s_hi;
    const EqBatchTab d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const uint32_t *f = factors + d.f_off;
    const unsigned t = threadIdx.x, nv = d.nv;
    const size_t base = (size_t)(blockIdx.x - d.first_wg) * MLE_BATCH_CHUNK;
    // H times 1 / R: out of Montgomery form once per workgroup instead of once per word
    me_chunk_weights(f, nv, base, t, 1u, s_u, s_a, s_b, &s_hi);
    const uint32_t w = mont_mul(mont_mul(s_a[t & 15], s_b[t >> 4]), s_hi);  // A B H, canonical
    if (d.n >= 4) {  // uniform over the workgroup
        // (the descriptor's pointer is a global address: said so, the store is one global_store_dwordx4 instead of flat halves)
        eq_v4u_global *p = (eq_v4u_global *)d.out;
        const size_t nq = d.n / 4, q0 = base / 4;
#pragma unroll
        for (int j = 0; j < ME_LOADS; j++) {
            const size_t q = q0 + (size_t)j * TPB + t;
            const uint4 u = reinterpret_cast<const uint4 *>(s_u)[j];  // uniform address: one LDS read per wave
            if (q < nq) p[q] = zk_v4u{mont_mul(u.x, w), mont_mul(u.y, w), mont_mul(u.z, w), mont_mul(u.w, w)};
        }
    } else if (t == 0) {  // one or two words: no 16 bytes to store (w = 1 here, the table has no variable above bit 0)
        for (unsigned c = 0; c < (unsigned)d.n; c++) d.out[c] = mont_mul(s_u[c], w);
    }
}

void launch_eq_batch_expand(const EqBatchTab *d_tabs, unsigned nt, unsigned nwg, const uint32_t *d_f, hipStream_t s) {
    hipLaunchKernelGGL(k_eq_batch_expand, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, d_f);
}

}  // namespace zk
