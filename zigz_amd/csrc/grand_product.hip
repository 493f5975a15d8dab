// Product trees of the grand-product argument: V_j[x] = V_{j+1}[x] * V_{j+1}[x + 2^j] (x < 2^j) for k independent columns
// (zigz_[dev_]product_layers_batch, zigz_[dev_]grand_product_prove_batch).  The HALVES pairing makes the two
// operands of a layer contiguous sub-arrays, so a lane that owns four consecutive x works on whole 16-byte vectors and a level
// needs no LDS and no cross-lane traffic.
//
//   k_gp_layers   one pass of up to three fused levels, one launch for all columns.  From layer J (m = 2^J words) a lane that owns
//                 the four consecutive x at 4 q < 2^(J - LEVELS) loads the 2^LEVELS vectors V_J[x + s 2^(J - LEVELS)] (non-temporal:
//                 the layer is read once), multiplies them pairwise -- vector s with vector s + 2^(LEVELS - 1), then the products
//                 with each other, the same pairs the levels form one by one -- and stores the layers J - 1 .. J - LEVELS as
//                 16-byte vectors.  mont_mul(to_mont(a), b): canonical in, canonical out.  With three levels fused a pass reads 4 m
//                 bytes and writes 3.5 m, where one level per launch moves 6 m per level.  No LDS, no atomics, no scratch, plain
//                 vector stores.  LEVELS is a template argument of the pass body and a field of the descriptor: the columns of one
//                 launch are at different heights (a 2^12 column takes one level while a 2^14 one takes three), so the kernel
//                 picks the instantiation per workgroup, uniformly.  The layout is the batched passes': a table of descriptors (GpTab), find_first_wg, a workgroup
//                 owns GP_CHUNK words of layer J, i.e. 8 >> LEVELS trips of 256 lanes; a layer shorter than a workgroup's share
//                 runs fewer trips (q < m / 2^LEVELS / 4 guards every trip).  Every load is below word m of the layer and every
//                 store inside its layer: 4 q + 3 + s 2^(J - LEVELS) < 2^(J - l) for the s < 2^(LEVELS - l) vectors of level l.
//   k_gp_top      one workgroup per column: from the first layer of at most 2048 words (the column itself when it is that short)
//                 down to layer 0 through LDS.  A lane's level-j word x reads s[x] and s[x + 2^j] and writes s[x]: nobody else
//                 touches either within the level, a barrier separates the levels.  Optionally every layer it holds, its input
//                 included, goes to pinned memory as well -- layer j at word 2^(J + 1) - 2^(j + 1) of the column's share -- and the
//                 launch signals completion (signal_done_block: fence, barrier, count), which hands the host the top of every
//                 tree in ONE hand-off.
#include "sop_dev.hpp"

namespace zk {

namespace {

__device__ __forceinline__ uint32_t gp_mul(uint32_t a, uint32_t b) { return mont_mul(to_mont(a), b); }
__device__ __forceinline__ uint4 gp_mul4(const uint4 &a, const uint4 &b) {
    return make_uint4(gp_mul(a.x, b.x), gp_mul(a.y, b.y), gp_mul(a.z, b.z), gp_mul(a.w, b.w));
}

static_assert(GP_CHUNK == 8 * 4 * TPB, "a workgroup's share of layer J: 8 >> LEVELS trips of 2^LEVELS vectors per lane");

template <int LEVELS>
__device__ __forceinline__ void gp_layers(const GpTab &d) {
    constexpr int TRIPS = 8 >> LEVELS, VECS = 1 << LEVELS;
    const uint64_t m = (uint64_t)1 << d.log2_in;
    const uint32_t nx = (uint32_t)(m >> LEVELS);  // words of layer J - LEVELS; a multiple of 2048
    const uint32_t nq = nx / 4;
    const uint32_t q0 = (blockIdx.x - d.first_wg) * (TRIPS * TPB) + threadIdx.x;
    const uint32_t *in = d.in;
    uint32_t *out[LEVELS];
#pragma unroll
    for (int l = 0; l < LEVELS; l++) out[l] = d.tree + (d.n - (m >> l));  // layer J - l - 1 at word n - 2^(J - l)
#pragma unroll 1
    for (int it = 0; it < TRIPS; it++) {
        const uint32_t q = q0 + (uint32_t)it * TPB;
        if (q < nq) {
            // byte offsets fit 32 bits: 16 q + 4 s nx < 4 m <= 2^32
            uint4 a[VECS];
#pragma unroll
            for (int s = 0; s < VECS; s++) a[s] = sop_load(in, 16 * q + 4 * nx * (uint32_t)s);
#pragma unroll
            for (int l = 0; l < LEVELS; l++) {
                const int cnt = VECS >> (l + 1);
#pragma unroll
                for (int s = 0; s < cnt; s++) {
                    a[s] = gp_mul4(a[s], a[s + cnt]);
                    sop_store16(out[l], 16 * q + 4 * nx * (uint32_t)s, a[s]);
                }
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(TPB) void k_gp_layers(const GpTab *__restrict__ tabs, unsigned nt) {
    const GpTab d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    switch (d.levels) {  // uniform over the workgroup
        case 1: gp_layers<1>(d); break;
        case 2: gp_layers<2>(d); break;
        default: gp_layers<3>(d); break;
    }
}

__global__ __launch_bounds__(TPB) void k_gp_top(const GpTop *__restrict__ tabs, uint32_t *h_dst, DoneFlag done) {
    __shared__ uint32_t s[1u << GP_TOP_LOG2];
    ZK_PRIO_SMALL();
    const GpTop d = tabs[blockIdx.x];
    const unsigned J = d.log2_in, t = threadIdx.x;
    uint32_t *top = h_dst ? h_dst + d.top_off : nullptr;
    for (unsigned i = t; i < (1u << J); i += TPB) {
        const uint32_t v = d.in[i];
        s[i] = v;
        if (top) top[i] = v;
    }
    __syncthreads();
    for (unsigned j = J; j-- > 0;) {
        const unsigned w = 1u << j, at = (2u << J) - (2u << j);
        uint32_t *dst = d.tree + (d.n - (2u << j));
        for (unsigned x = t; x < w; x += TPB) {
            const uint32_t p = gp_mul(s[x], s[x + w]);
            s[x] = p;
            dst[x] = p;
            if (top) top[at + x] = p;
        }
        __syncthreads();
    }
    signal_done_block(done, gridDim.x);  // (TPB threads: several waves; no thread returns early)
}

void launch_gp_layers(const GpTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_gp_layers, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}
void launch_gp_top(const GpTop *d_tabs, unsigned nt, uint32_t *h_dst, hipStream_t s, DoneFlag done) {
    hipLaunchKernelGGL(k_gp_top, dim3(nt), dim3(TPB), 0, s, d_tabs, h_dst, done);
}

}  // namespace zk
