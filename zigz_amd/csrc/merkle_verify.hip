// Batched Merkle verification: SimpleMerkleTree.verify (merkle_tree.zig:362-373) for k independent openings in shared
// launches.
//
// An opening is a chain of height + 1 dependent permutations -- hashLeaf(value), then one hashInternal per level -- and the
// openings are independent, so a lane takes one opening from leaf to root.  The host sorts the openings by height into
// buckets (MVerifyTab, kernels.hpp); a bucket owns whole workgroups, found by a binary search over the first_wg prefix like
// the batched trees' descriptors (merkle_batch.hip), so every wave walks the same number of levels and no lane idles through
// levels it does not have.
//
// Siblings arrive as canonical SHA3 bytes and are turned into the tree form of keccak.hpp on load; the chain stays in tree
// form and only its end is turned back into bytes, for the comparison with the root.  The host form stages each bucket's
// siblings level-major (level l of all its lanes contiguous), so a wave's 32-byte loads of one level coalesce; the device
// form reads the caller's packed layout as given.
//
// A lane writes its verdict byte straight into pinned memory at the caller's index; a wave counts its rejects with one
// atomic add.  The verdicts are fenced system-wide before the launch ends; the reject count reaches the host through the
// publish launch queued behind the last verify launch of a call (k_publish, which fences, passes a barrier and counts).
#include "kernels.hpp"

#include "tree_dev.hpp"

namespace zk {

static_assert(MV_TPB == TPB, "the host sizes the grid in workgroups of TPB threads");

namespace {

// canonical SHA3 bytes (4 little-endian u64 lanes) -> tree form: even bits of each lane in the low word, odd bits in the high
// word (the inverse of canonical_digest)
__device__ __forceinline__ uint64_t tree_lane(uint64_t x) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    const uint32_t e = compress_even(lo) | (compress_even(hi) << 16);
    const uint32_t o = compress_even(lo >> 1) | (compress_even(hi >> 1) << 16);
    return ((uint64_t)o << 32) | e;
}
__device__ __forceinline__ Digest load_tree_form(const uint8_t *p) {
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(p);
    const ulonglong2 x = q[0], y = q[1];
    return Digest{{tree_lane(x.x), tree_lane(x.y), tree_lane(y.x), tree_lane(y.y)}};
}

}  // namespace

// One lane per opening.  DEV: the device form (gathers through order / soff from the caller's layout); PAUSE: the hash with
// the re-arm pauses, for launches that fill the chip.
template <bool DEV, bool PAUSE>
__global__ __launch_bounds__(TPB) void k_mverify(const MVerifyTab *__restrict__ tabs, unsigned nt, MVerifyArgs a) {
    const MVerifyTab &t = tabs[find_first_wg(tabs, nt, blockIdx.x)];
    const unsigned i = (blockIdx.x - t.first_wg) * TPB + threadIdx.x;  // lane within the bucket
    const bool active = i < t.cnt;
    bool ok = true;
    if (active) {
        const size_t j = t.base + i;  // sorted position
        const uint32_t orig = a.order[j - a.lo];
        const size_t src = DEV ? orig : j - a.lo;
        Digest cur = sha3_leaf<PAUSE>(a.vals[src]);  // hashLeaf: the value's 8 little-endian bytes, as given
        const unsigned h = t.height, cnt = t.cnt;
        const uint8_t *sp = DEV ? a.sib + (size_t)a.soff[j] * 32 : t.sib + (size_t)i * 32;
        const uint8_t *dp = DEV ? a.dirs + a.soff[j] : t.dirs + i;
        const size_t sstep = DEV ? 32 : (size_t)cnt * 32, dstep = DEV ? 1 : cnt;
#pragma unroll 1
        for (unsigned l = 0; l < h; l++) {
            const Digest s = load_tree_form(sp);
            const bool right = *dp != 0;  // is_right: the sibling is on the left
            Digest L, R;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                L.w[w] = right ? s.w[w] : cur.w[w];
                R.w[w] = right ? cur.w[w] : s.w[w];
            }
            cur = sha3_node<PAUSE>(L, R);
            sp += sstep;
            dp += dstep;
        }
        const Digest c = canonical_digest(cur);
        const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(a.roots + src * 32);
        const ulonglong2 r0 = r[0], r1 = r[1];
        ok = c.w[0] == r0.x && c.w[1] == r0.y && c.w[2] == r1.x && c.w[3] == r1.y;
        a.verdicts[orig] = ok ? 1 : 0;
    }
    const unsigned long long rej = __ballot(active && !ok);
    if ((threadIdx.x & 63) == 0 && rej) atomicAdd(a.rejected, (unsigned long long)__popcll(rej));
    __threadfence_system();  // the verdicts reach pinned memory before the launch ends
}

void launch_mverify(const MVerifyTab *d_tabs, unsigned nt, unsigned nwg, const MVerifyArgs &a, bool dev, bool pause, hipStream_t s) {
    if (dev) {
        if (pause) hipLaunchKernelGGL((k_mverify<true, true>), dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, a);
        else hipLaunchKernelGGL((k_mverify<true, false>), dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, a);
    } else {
        if (pause) hipLaunchKernelGGL((k_mverify<false, true>), dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, a);
        else hipLaunchKernelGGL((k_mverify<false, false>), dim3(nwg), dim3(TPB), 0, s, d_tabs, nt, a);
    }
}

}  // namespace zk
