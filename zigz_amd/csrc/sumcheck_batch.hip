// Batched radix sumcheck passes: several independent tables of different lengths in ONE launch per pass.
//
// The single-table kernels (kernels.hip: k_block_sums, k_radix_fold, k_radix_finalize) batch over equal-length columns
// with one stride.  A batch of proofs has tables of any power-of-two length, so each launch here reads a small table of
// per-table descriptors (BatchTab, kernels.hpp) and every workgroup finds its table by a binary search over the prefix
// of workgroup counts.  Exact u64 sums, non-temporal streaming loads and the deferred Montgomery reduction are those of
// the single kernels, so every table's sums and folded values are bit-identical to a run of its own.
//
// Results reach the host through pinned memory: a pass's sums (or the tails) are written there by one launch in which every
// workgroup writes its share, fences system-wide and passes a barrier BEFORE it counts itself, so no wave's stores can trail
// the count; the last workgroup stores the completion word.  (One workgroup copying all sums of 16 tables at the end of the
// block-sums launch took ~0.4 ms: 16 K host writes from one CU.)
#include "kernels.hpp"

#include "field.hpp"
#include "tree_dev.hpp"

namespace zk {

static_assert(BATCH_WG == TPB, "the batch launchers count workgroups of TPB threads");

namespace {

constexpr int B_INFLIGHT = 4;  // 16-byte loads in flight per lane in the block-sums pass (k_block_sums: ZK_BS_INFLIGHT)
constexpr int B_RB = 16;       // rows per chunk of the fold (k_radix_fold: RB)
constexpr int B_RLOOPS = 4;    // chunks per thread (k_radix_fold: RLOOPS) -> 64 rows per workgroup row-group

template <bool FULL>
__device__ __forceinline__ void b_fold_rows(const uint4 *p, const uint32_t *__restrict__ w, size_t mq, size_t nb, size_t gy,
                                            unsigned long long lo[4], unsigned long long hi[4]) {
#pragma unroll 1
    for (int l = 0; l < B_RLOOPS; l++) {
        const size_t b0 = (gy * B_RLOOPS + l) * B_RB;
        if (!FULL && b0 >= nb) break;
        uint4 v[B_RB];
#pragma unroll
        for (int j = 0; j < B_RB; j++) v[j] = stream_load(p + (FULL || b0 + j < nb ? b0 + j : nb - 1) * mq);
#pragma unroll
        for (int j = 0; j < B_RB; j++) {
            const uint32_t wj = FULL ? w[b0 + j] : (w[b0 + j < nb ? b0 + j : nb - 1] & (b0 + j < nb ? ~0u : 0u));
            const uint32_t e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const unsigned long long pr = (unsigned long long)wj * e[c];
                lo[c] += (uint32_t)pr;
                hi[c] += pr >> 32;
            }
        }
    }
}

// XXH3-64 of one u64 (k_lasso_fingerprints' row step, kernels.hip)
__device__ __forceinline__ uint64_t b_xxh3_64_of_u64(uint64_t h) {
    const uint64_t bitflip = 0x1cad21f72c81017cull ^ 0xdb979083e96dd4deull;  // kSecret[8..16) ^ kSecret[16..24)
    const uint64_t in64 = (h >> 32) + (h << 32);
    uint64_t k = in64 ^ bitflip;
    k ^= ((k << 49) | (k >> 15)) ^ ((k << 24) | (k >> 40));
    k *= 0x9FB21C651E98DF25ull;
    k ^= (k >> 35) + 8;
    k *= 0x9FB21C651E98DF25ull;
    return k ^ (k >> 28);
}

}  // namespace

// Pass 1 of a stage: the 2^k exact block sums of every table.  A wave reads iters x 64 16-byte chunks inside one block and
// adds one partial sum; the pass's sums of all tables are one contiguous array (k_batch_publish hands it to the host).
__global__ __launch_bounds__(TPB) void k_batch_block_sums(const BatchTab *__restrict__ tabs, unsigned nt) {
    const BatchTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const unsigned lane = threadIdx.x & 63;
    const size_t wave = (size_t)(blockIdx.x - d.first_wg) * (TPB / 64) + (threadIdx.x >> 6);
    const unsigned iters = d.iters;
    const size_t chunks = ((size_t)1 << d.log2_n) / 4;
    const size_t c0 = wave * (size_t)iters * 64;
    unsigned long long acc = 0;
    if (c0 < chunks) {  // wave-uniform
        const uint4 *p = reinterpret_cast<const uint4 *>(d.in) + c0 + lane;
#pragma unroll 1
        for (unsigned it = 0; it < iters; it += B_INFLIGHT) {
            uint4 a[B_INFLIGHT];
#pragma unroll
            for (int j = 0; j < B_INFLIGHT; j++) a[j] = stream_load(p + (size_t)(it + j < iters ? it + j : iters - 1) * 64);
#pragma unroll
            for (int j = 0; j < B_INFLIGHT; j++)
                acc += it + j < iters ? (unsigned long long)a[j].x + a[j].y + a[j].z + a[j].w : 0ull;
        }
        acc = wave_sum(acc);
        if (lane == 0 && acc) atomicAdd(&d.sums[(c0 * 4) >> (d.log2_n - d.k)], acc);
    }
}

// Pass 2a: part[g][i] = sum over the g-th group of 64 rows b of W[b] * T[b*m + i]  (exact u64, m = n / 2^k), as k_radix_fold.
__global__ __launch_bounds__(TPB) void k_batch_fold(const BatchTab *__restrict__ tabs, unsigned nt) {
    ZK_PRIO_SMALL();
    const BatchTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const size_t m = (size_t)1 << (d.log2_n - d.k), nb = (size_t)1 << d.k, mq = m / 4;
    const size_t gx = (mq + TPB - 1) / TPB;
    const size_t local = blockIdx.x - d.first_wg, gy = local / gx;
    const size_t q = (local - gy * gx) * TPB + threadIdx.x;  // uint4 index of the outputs
    if (q >= mq) return;
    const uint4 *p = reinterpret_cast<const uint4 *>(d.in) + q;
    unsigned long long lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    if (nb % ((size_t)B_RB * B_RLOOPS) == 0) b_fold_rows<true>(p, d.w, mq, nb, gy, lo, hi);
    else b_fold_rows<false>(p, d.w, mq, nb, gy, lo, hi);
    unsigned long long s[4];
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = hi[c] + monty_reduce(lo[c]);  // lo < 2^38 < p * 2^32
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(d.part + gy * m + q * 4);
    o[0] = make_ulonglong2(s[0], s[1]);
    o[1] = make_ulonglong2(s[2], s[3]);
}

// Pass 2b: out[i] = (sum_g part[g][i]) mod p; tables with a next stage add its block sums (blocks of 2^log2_m2 >= 256 outputs:
// the 64 outputs of a wave fall into one block).  The next stage's sums of all tables form one contiguous array.
__global__ __launch_bounds__(TPB) void k_batch_finalize(const BatchTab *__restrict__ tabs, unsigned nt) {
    ZK_PRIO_SMALL();
    const BatchTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const size_t m = (size_t)1 << (d.log2_n - d.k), groups = ((size_t)1 << d.k) > (size_t)B_RB * B_RLOOPS
                                                                   ? ((size_t)1 << d.k) / ((size_t)B_RB * B_RLOOPS) : 1;
    const size_t i = (size_t)(blockIdx.x - d.first_wg) * TPB + threadIdx.x;
    uint32_t v = 0;
    if (i < m) {
        const unsigned long long *pp = d.part + i;
        unsigned long long t = 0;
        for (size_t g = 0; g < groups; g++) t += pp[g * m];
        v = (uint32_t)(t % (unsigned long long)P);
        d.out[i] = v;
    }
    if (d.log2_m2) {  // uniform over the workgroup (one table per workgroup)
        const unsigned long long t = wave_sum((unsigned long long)v);
        if ((threadIdx.x & 63) == 0 && i < m && t) atomicAdd(&d.sums[i >> d.log2_m2], t);
    }
}

// completion of a launch whose workgroups each wrote their share into pinned memory
__device__ __forceinline__ void b_count_done(const BatchPublish &pub) {
    __shared__ int s_last;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(pub.count, 1u) == gridDim.x - 1;
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence_system();
        *pub.count = 0;
        __hip_atomic_store(pub.flag, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// A pass's n sums (u64, written by the launch before on the same stream) into pinned memory, left zero for the next pass.
__global__ __launch_bounds__(TPB) void k_batch_publish(BatchPublish pub) {
    const size_t j = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (j < pub.n) {
        reinterpret_cast<unsigned long long *>(pub.h_dst)[j] = pub.d_sums[j];
        pub.d_sums[j] = 0;
    }
    b_count_done(pub);
}

// The remaining tables (<= 1024 values each) into pinned memory, u32, table j's at pub.h_dst + tail_off words: every workgroup
// writes its share, fences system-wide and passes a barrier before it counts itself; the last one stores the completion word.
__global__ __launch_bounds__(TPB) void k_batch_tails(const BatchTab *__restrict__ tabs, unsigned nt, BatchPublish pub) {
    const BatchTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const size_t m = (size_t)1 << d.log2_n;
    const size_t i = (size_t)(blockIdx.x - d.first_wg) * TPB + threadIdx.x;
    if (i < m) reinterpret_cast<uint32_t *>(pub.h_dst)[d.tail_off + i] = d.in[i];
    b_count_done(pub);
}

// Lasso fingerprints of several instances' rows in one launch (k_lasso_fingerprints per row, per-instance widths): table t's
// rows at in, its fingerprints at out; rows past `rows` up to the padded count are written as 0 (lasso_prover.zig:139-142).
__global__ __launch_bounds__(TPB) void k_batch_fingerprints(const FpTab *__restrict__ tabs, unsigned nt) {
    const FpTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const size_t i = (size_t)(blockIdx.x - d.first_wg) * TPB + threadIdx.x;
    if (i >= d.padded) return;
    if (i >= d.rows) {
        d.out[i] = 0;
        return;
    }
    uint64_t h = 0;
    for (unsigned f = 0; f < d.width; f++) {
        h ^= d.in[i * d.width + f];
        h = b_xxh3_64_of_u64(h);
    }
    d.out[i] = (uint32_t)(h % (uint64_t)P);
}

void launch_batch_block_sums(const BatchTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_block_sums, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}
void launch_batch_fold(const BatchTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_fold, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}
void launch_batch_finalize(const BatchTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_finalize, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}
void launch_batch_publish(const BatchPublish &pub, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_publish, dim3((unsigned)((pub.n + TPB - 1) / TPB)), dim3(TPB), 0, s, pub);
}
void launch_batch_tails(const BatchTab *d_tabs, unsigned nt, unsigned nwg, const BatchPublish &pub, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_tails, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, pub);
}
void launch_batch_fingerprints(const FpTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_fingerprints, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}

}  // namespace zk
