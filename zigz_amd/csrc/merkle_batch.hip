// Batched Merkle trees: k independent SimpleMerkleTree builds and openings in shared launches.
//
// The dense single-tree path (kernels.hip: k_keccak_leaves, k_keccak_level, k_merkle_top) takes one launch per level of ONE
// tree, so a batch of small trees would be launches and round trips only.  Here every launch serves every tree that has work
// at that step: it reads a table of per-tree descriptors (MBatchTab, kernels.hpp) and every workgroup finds its tree by a
// binary search over the prefix of workgroup counts, as the batched sumcheck does (sumcheck_batch.hip).
//
// A build runs in stages.  A stage-s workgroup takes a block of up to MB_BLOCK (512) nodes of level 9 s -- in stage 0 the
// leaves, which it hashes from the values (pad leaves are hashLeaf(0)) -- and computes the levels above the block in LDS, one
// barrier per level, writing every node it computes into the tree (slab_tree_ref's node layout).  A tree of 512 leaves or fewer
// is complete after stage 0; a batch needs ceil(height / 9) stages for its highest tree, however many trees it holds.
// Digests stay in the tree form of keccak.hpp and become canonical bytes only where they leave the device (roots, paths).
//
// An opening is one wave per tree (k_mbatch_paths).  A CommitmentScheme opening evaluates the tables first with the batched
// MLE kernels (mle_batch.hip: k_mle_batch_eval, k_mle_batch_finish) into result words in the handle, which the path launch
// copies out: this file has no evaluation of its own.
//
// Results reach the host through pinned memory: every workgroup of a publishing launch writes its share, fences system-wide
// and passes a barrier BEFORE it counts itself (signal_done_block, tree_dev.hpp); the last one stores the completion word.
#include "kernels.hpp"

#include "field.hpp"
#include "tree_dev.hpp"

namespace zk {

static_assert(MB_BLOCK == 1u << MB_STAGE_LEVELS, "a stage's block spans its levels");
static_assert(MB_BLOCK == 2 * TPB, "a stage-0 workgroup hashes two leaves per thread");

namespace {

// The levels above a block of `cnt` digests (a power of two <= MB_BLOCK) of level l that sit in A; the block's first node is
// node `base` of level l.  Ping-pong between A and B: a level reads one buffer and writes the other, so one barrier per level
// suffices.  Every thread of the workgroup calls this (cnt is uniform).
__device__ __forceinline__ void mb_levels(Digest *A, Digest *B, uint8_t *tree, size_t npad, unsigned l, size_t base, unsigned cnt) {
    Digest *in = A, *out = B;
#pragma unroll 1
    for (unsigned c = cnt; c > 1; c >>= 1) {
        __syncthreads();
        const unsigned half = c >> 1;
        l++;
        base >>= 1;
        if (threadIdx.x < half) {
            const Digest d = sha3_node(in[2 * threadIdx.x], in[2 * threadIdx.x + 1]);
            out[threadIdx.x] = d;
            store_digest(tree, slab_level_offset(npad, l) + base + threadIdx.x, d);
        }
        Digest *t = in;
        in = out;
        out = t;
    }
}

}  // namespace

// Stage 0: the leaves of a block of up to 512 (two per thread), then the levels above it.  The values are copied into the
// handle on the way (src != vals: a device batch; the host batch uploads straight into the handle).
__global__ __launch_bounds__(TPB) void k_mbatch_subtrees(const MBatchTab *__restrict__ tabs, unsigned nt) {
    __shared__ __align__(16) Digest A[MB_BLOCK];
    __shared__ __align__(16) Digest B[MB_BLOCK / 2];
    const MBatchTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const size_t base = (size_t)(blockIdx.x - d.first_wg) * MB_BLOCK;
    const unsigned cnt = (unsigned)(d.npad - base < MB_BLOCK ? d.npad - base : MB_BLOCK);
    const bool copy = d.src != d.vals;
#pragma unroll 1
    for (unsigned e = threadIdx.x; e < cnt; e += TPB) {
        const size_t i = base + e;
        uint64_t x = 0;  // pad with hashLeaf(0), merkle_tree.zig:302-306
        if (i < d.n) {
            const uint32_t v = d.src[i];
            if (copy) d.vals[i] = v;
            x = v;
        }
        const Digest g = sha3_leaf(x);
        A[e] = g;
        store_digest(d.tree, i, g);
    }
    mb_levels(A, B, d.tree, d.npad, 0, base, cnt);
}

// Stage s > 0: a block of up to 512 nodes of level lin = 9 s, fetched with coalesced 16-byte loads into LDS, then the levels
// above it.
__global__ __launch_bounds__(TPB) void k_mbatch_level(const MBatchTab *__restrict__ tabs, unsigned nt) {
    __shared__ __align__(16) Digest A[MB_BLOCK];
    __shared__ __align__(16) Digest B[MB_BLOCK / 2];
    const MBatchTab &d = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const size_t n_in = d.npad >> d.lin, base = (size_t)(blockIdx.x - d.first_wg) * MB_BLOCK;
    const unsigned cnt = (unsigned)(n_in - base < MB_BLOCK ? n_in - base : MB_BLOCK);
    const uint4 *g = reinterpret_cast<const uint4 *>(d.tree + (slab_level_offset(d.npad, d.lin) + base) * 32);
    uint4 *a = reinterpret_cast<uint4 *>(A);
#pragma unroll 1
    for (unsigned c = threadIdx.x; c < 2 * cnt; c += TPB) a[c] = g[c];
    mb_levels(A, B, d.tree, d.npad, d.lin, base, cnt);
}

// The k roots (node 2 npad - 2 of each tree), canonical bytes, into pinned memory at h_roots + 32 idx.
__global__ __launch_bounds__(TPB) void k_mbatch_roots(const MBatchTab *__restrict__ tabs, unsigned nt, uint8_t *h_roots, DoneFlag done) {
    const unsigned j = blockIdx.x * TPB + threadIdx.x;
    if (j < nt) {
        const MBatchTab &d = tabs[j];
        const Digest r = canonical_digest(load_digest(d.tree, 2 * d.npad - 2));  // tree form -> SHA3 bytes
        ulonglong2 *q = reinterpret_cast<ulonglong2 *>(h_roots + (size_t)d.idx * 32);
        q[0] = make_ulonglong2(r.w[0], r.w[1]);
        q[1] = make_ulonglong2(r.w[2], r.w[3]);
    }
    signal_done_block(done, gridDim.x);  // (TPB threads: several waves; no thread returns early)
}

// tree.open(index) of every tree (merkle_tree.zig:324-360), one wave per tree, lane l for level l; the paths, the leaves and
// the evaluations (reduced results of k_mle_batch_finish, queued in front of this launch) go straight into pinned memory.
__global__ __launch_bounds__(64) void k_mbatch_paths(const MPathTab *__restrict__ tabs, unsigned nt, MPathOut out, DoneFlag done) {
    ZK_PRIO_SMALL();
    const MPathTab &d = tabs[blockIdx.x];
    const unsigned l = threadIdx.x;
    if (l == 0) {
        out.leaf[d.idx] = d.vals[d.index];
        if (d.acc) out.value[d.idx] = *d.acc;
    }
    if (l < d.height) {
        const size_t ci = d.index >> l;  // current_index at level l
        const Digest g = canonical_digest(load_digest(d.tree, slab_level_offset(d.npad, l) + (ci ^ 1)));
        ulonglong2 *q = reinterpret_cast<ulonglong2 *>(out.sib + (d.sib_off + l) * 32);
        q[0] = make_ulonglong2(g.w[0], g.w[1]);
        q[1] = make_ulonglong2(g.w[2], g.w[3]);
        out.dirs[d.sib_off + l] = (uint8_t)(ci & 1);  // directions[l] = is_right
    }
    signal_done_block(done, gridDim.x);
}

// Many openings of the batch's trees (zigz_merkle_open_many): any number per tree, in the caller's order.  The work item is 16
// bytes of one sibling digest: a workgroup owns TPB / 2 consecutive sibling slots of the packed output, consecutive lanes store
// consecutive 16 bytes, and the reads from the trees are the scattered side.  The workgroup finds the openings of its first and
// last slot by a binary search over the descriptors' slot offsets (uniform: scalar loads), a lane its own opening between the
// two.  Openings of height 0 share their offset with the opening after them: the LAST descriptor whose offset is <= the slot
// owns it.  The lanes of an opening's level 0 also write its leaf value and root; an opening without siblings has no such
// lane, so the workgroups behind the sibling workgroups take one opening per thread and serve those.
__device__ __forceinline__ unsigned mo_find(const mo::Desc *__restrict__ desc, unsigned lo, unsigned hi, unsigned slot) {
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (desc[mid].off <= slot) lo = mid;
        else hi = mid;
    }
    return lo;
}
template <bool NT>
__device__ __forceinline__ void mo_store16(uint8_t *p, const uint4 &v) {
    if (NT) nt_store16(reinterpret_cast<uint4 *>(p), v);
    else *reinterpret_cast<uint4 *>(p) = v;
}
template <bool NT>
__global__ __launch_bounds__(TPB) void k_mbatch_open_many(const MOpenTree *__restrict__ trees, const mo::Desc *__restrict__ desc,
                                                          unsigned k, unsigned slots, unsigned sib_wgs, MOpenOut out, DoneFlag done) {
    if (blockIdx.x < sib_wgs) {
        const unsigned s0 = blockIdx.x * (TPB / 2);
        const unsigned s1 = (slots - s0 < TPB / 2 ? slots : s0 + TPB / 2) - 1;
        const unsigned j0 = mo_find(desc, 0, k, s0), j1 = mo_find(desc, j0, k, s1);
        const unsigned slot = s0 + (threadIdx.x >> 1), half = threadIdx.x & 1;
        if (slot <= s1) {
            const unsigned j = mo_find(desc, j0, j1 + 1, slot);
            const mo::Desc d = desc[j];
            const MOpenTree T = trees[d.tree];
            const unsigned l = slot - d.off;
            const uint64_t ci = d.index >> l;  // current_index at level l; its sibling is node ci ^ 1
            const uint4 v = canonical_half(T.tree + (slab_level_offset(T.npad, l) + (ci ^ 1)) * 32 + half * 16);
            mo_store16<NT>(out.sib + (size_t)slot * 32 + half * 16, v);
            if (!half) out.dirs[slot] = (uint8_t)(ci & 1);  // directions[l] = is_right
            if (l == 0) {
                if (!half) out.leaf[j] = T.vals[d.index];
                if (out.roots) mo_store16<NT>(out.roots + (size_t)j * 32 + half * 16, canonical_half(T.tree + (2 * T.npad - 2) * 32 + half * 16));
            }
        }
    } else {
        const unsigned j = (blockIdx.x - sib_wgs) * TPB + threadIdx.x;
        if (j < k) {
            const mo::Desc d = desc[j];
            const MOpenTree T = trees[d.tree];
            if (T.height == 0) {  // one leaf: it is the root
                out.leaf[j] = T.vals[d.index];
                if (out.roots) {
                    mo_store16<NT>(out.roots + (size_t)j * 32, canonical_half(T.tree));
                    mo_store16<NT>(out.roots + (size_t)j * 32 + 16, canonical_half(T.tree + 16));
                }
            }
        }
    }
    signal_done_block(done, gridDim.x);
}

void launch_mbatch_subtrees(const MBatchTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_mbatch_subtrees, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}
void launch_mbatch_level(const MBatchTab *d_tabs, unsigned nt, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL(k_mbatch_level, dim3(nwg), dim3(TPB), 0, s, d_tabs, nt);
}
void launch_mbatch_roots(const MBatchTab *d_tabs, unsigned nt, uint8_t *h_roots, hipStream_t s, DoneFlag done) {
    hipLaunchKernelGGL(k_mbatch_roots, dim3((nt + TPB - 1) / TPB), dim3(TPB), 0, s, d_tabs, nt, h_roots, done);
}
void launch_mbatch_paths(const MPathTab *d_tabs, unsigned nt, const MPathOut &out, hipStream_t s, DoneFlag done) {
    hipLaunchKernelGGL(k_mbatch_paths, dim3(nt), dim3(64), 0, s, d_tabs, nt, out, done);
}

void launch_mbatch_open_many(const MOpenTree *d_trees, const mo::Desc *d_desc, unsigned k, unsigned slots, bool zero_height,
                             const MOpenOut &out, bool nt, hipStream_t s, DoneFlag done) {
    const unsigned sib_wgs = (slots + TPB / 2 - 1) / (TPB / 2), grid = sib_wgs + (zero_height ? (k + TPB - 1) / TPB : 0);
    if (nt) hipLaunchKernelGGL(k_mbatch_open_many<true>, dim3(grid), dim3(TPB), 0, s, d_trees, d_desc, k, slots, sib_wgs, out, done);
    else hipLaunchKernelGGL(k_mbatch_open_many<false>, dim3(grid), dim3(TPB), 0, s, d_trees, d_desc, k, slots, sib_wgs, out, done);
}

}  // namespace zk
