// Batched MLE evaluation over free-standing tables: k independent Multilinear.eval calls (multilinear.zig:110-144) in ONE launch.
//
// eval(point) = sum_i T[i] * prod_v f_v[bit v of i], f_v = (1 - r_v, r_v), r_v the coordinate bound to index bit v.  The launch
// reads a table of per-pair descriptors (MleBatchTab, kernels.hpp); every workgroup finds its pair by a binary search over the
// prefix of workgroup counts, as the batched sumcheck and the batched Merkle builds do, and owns one chunk of MLE_BATCH_CHUNK
// (8192) consecutive elements of that pair's table: 8 streaming 16-byte loads per lane, issued back to back.
//
// The weight of element i factors along its index bits, and the chunk layout i = base + 4 (256 j + thread) + c splits them into
//   bits  0-1  c       and bits 10-12  j : 32 workgroup-uniform weights U[j][c], built once per workgroup in LDS
//   bits  2-9  thread                    : two 16-entry tables A (bits 2-5), B (bits 6-9) in LDS, one product per lane
//   bits 13+   workgroup                 : one uniform factor H (a product over the lanes of one wave)
// so a lane forms  sum_{j,c} U[j][c] * T[..]  with ONE widening multiply per element and no reduction inside the loop (32-bit
// multiplies issue at under half rate on gfx950; see k_radix_fold): U is in Montgomery form (u R), the 64-bit products are added
// as separate low and high halves, and  hi + monty_reduce(lo)  is congruent to  sum u T  (k_radix_fold's deferred reduction).
// One Montgomery reduction and one multiply by the lane's weight A B H turn that into the lane's term.  A variable past the
// table's own (a table smaller than a chunk) has the factor pair (1, 0): every element that does not exist gets weight 0 and
// its load is clamped to the chunk's first 16 bytes.
//
// Exact arithmetic: every lane term is a canonical product below p; a pair's terms -- at most one per 32 elements, at least
// one -- are added in u64: a shuffle sum per wave, the four waves through LDS, and ONE plain store per workgroup into a
// partial array indexed by the workgroup's number (no atomics: with one accumulator per pair the 512 .. 2048 waves of a
// 2^20 .. 2^22 table queued up behind one cache line, and the launch ran at a tenth of the HBM rate).  k_mle_batch_finish, one
// workgroup per pair, adds the pair's partials, reduces mod p ONCE and writes the result at the pair's slot: into pinned memory,
// signalling the host afterwards (signal_done_block: fence, barrier, then count), or, for a batch opening
// (zigz_commit_open_batch), into device words that the path launch behind it reads, signalling nothing.  With
// n <= 2^MLE_BATCH_MAX_LOG2_N a pair's sum stays below 2^31 * n <= 2^63 and cannot wrap.  Every partial is written by every
// launch, so nothing has to be zeroed between calls.
#include "mle_batch_dev.hpp"  // the chunk's weights U, A, B, H (shared with k_eq_batch_expand, eq_batch.hip)

namespace zk {

static_assert(31 + MLE_BATCH_MAX_LOG2_N < 64, "a pair's exact u64 sum: fewer than n terms below p < 2^31");

__global__ __launch_bounds__(TPB) void k_mle_batch_eval(const MleBatchTab *__restrict__ tabs, unsigned nt,
                                                        const uint32_t *__restrict__ factors, unsigned long long *__restrict__ part) {
    ZK_PRIO_SMALL();
    __shared__ __align__(16) uint32_t s_u[4 * ME_LOADS];
    __shared__ uint32_t s_a[16], s_b[16], s_hi;
    __shared__ unsigned long long s_sum[TPB / 64];
    const MleBatchTab d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const uint32_t *f = factors + d.f_off;
    const unsigned t = threadIdx.x, nv = d.nv;
    const size_t base = (size_t)(blockIdx.x - d.first_wg) * MLE_BATCH_CHUNK;
    // one more factor R on H: the lane's sum arrives divided by R (monty_reduce below)
    me_chunk_weights(f, nv, base, t, R2_MOD_P, s_u, s_a, s_b, &s_hi);
    unsigned long long lo = 0, hi = 0;
    if (d.n >= 4) {  // uniform over the workgroup
        const uint4 *p = reinterpret_cast<const uint4 *>(d.vals);
        const size_t nq = d.n / 4, q0 = base / 4;
        uint4 v[ME_LOADS];
#pragma unroll
        for (int j = 0; j < ME_LOADS; j++) {
            const size_t q = q0 + (size_t)j * TPB + t;
            v[j] = stream_load(p + (q < nq ? q : q0));  // clamped, not branched: the loads are issued back to back
        }
#pragma unroll
        for (int j = 0; j < ME_LOADS; j++) {
            const uint4 u = reinterpret_cast<const uint4 *>(s_u)[j];  // uniform address: one LDS read per wave
            const uint32_t uu[4] = {u.x, u.y, u.z, u.w}, e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const unsigned long long pr = (unsigned long long)uu[c] * e[c];
                lo += (uint32_t)pr;
                hi += pr >> 32;
            }
        }
    } else if (t == 0) {  // one or two elements: no 16 bytes to load
        for (unsigned c = 0; c < (unsigned)d.n; c++) {
            const unsigned long long pr = (unsigned long long)s_u[c] * d.vals[c];
            lo += (uint32_t)pr;
            hi += pr >> 32;
        }
    }
    // lo < 32 * 2^32 and hi < 32 * 2^31: hi + monty_reduce(lo) < 2^37 is congruent to sum u T; reduced once more it is that sum / R
    const uint32_t s = monty_reduce(hi + monty_reduce(lo));
    const uint32_t w = mont_mul(mont_mul(s_a[t & 15], s_b[t >> 4]), s_hi);  // A B H R^2
    unsigned long long term = mont_mul(w, s);                               // canonical, < p
    term = wave_sum(term);
    if ((t & 63) == 0) s_sum[t >> 6] = term;
    __syncthreads();
    if (t == 0) part[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// One workgroup per pair: the pair's partial sums (one per workgroup of the eval launch, consecutive) added up, reduced mod p
// once and written at the pair's result slot: pinned memory (zigz_[dev_]mle_eval_batch, the sumcheck verifier) or the device
// words a batch opening's path launch reads (zigz_commit_open_batch, which signals nothing here: done.flag is null).
__global__ __launch_bounds__(TPB) void k_mle_batch_finish(const MleBatchTab *__restrict__ tabs, const unsigned long long *__restrict__ part,
                                                          uint64_t *out, DoneFlag done) {
    __shared__ unsigned long long s_sum[TPB / 64];
    const MleBatchTab d = tabs[blockIdx.x];
    const size_t cnt = (size_t)((d.n + MLE_BATCH_CHUNK - 1) / MLE_BATCH_CHUNK);
    const unsigned long long *p = part + d.first_wg;
    unsigned long long sum = 0;
    for (size_t j = threadIdx.x; j < cnt; j += TPB) sum += p[j];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) out[d.slot] = (s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]) % (unsigned long long)P;
    signal_done_block(done, gridDim.x);  // (TPB threads: several waves; no thread returns early)
}

void launch_mle_batch_eval(const MleBatchTab *d_tabs, unsigned nt, unsigned nwg, const uint32_t *d_f, unsigned long long *d_part,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_mle_batch_eval, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, d_f, d_part);
}
void launch_mle_batch_finish(const MleBatchTab *d_tabs, unsigned nt, const unsigned long long *d_part, uint64_t *out, hipStream_t s,
                             DoneFlag done) {
    hipLaunchKernelGGL(k_mle_batch_finish, dim3(nt), dim3(TPB), 0, s, d_tabs, d_part, out, done);
}

}  // namespace zk
