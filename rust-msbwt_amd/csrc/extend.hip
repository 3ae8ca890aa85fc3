// gfx950 (MI355X, CDNA4): left-extension counts from FM ranges -- the second phase of msbwt_rle_count_kmer_extensions.
//
// The range [l, h) of a k-mer q already holds the counts of the six (k+1)-mers c . q:
//     count(c . q) = (start_index[c] + rank_c(h)) - (start_index[c] + rank_c(l)),   c = 0..5 ($ A C G N T),
// one constrain_range (msbwt_core.rs:99) per symbol on the same two bounds.  A plane block (plane_index.hpp) carries all six
// symbols' bounds and the three bit planes in one 128-byte line, so the six counts cost the line of l -- and of h only when h lies
// in another block; a present k-mer's narrow range mostly lies in one.
//
// One 8-lane group per query, as constrain() in rank_ops.hpp: lane j loads chunk j of each line (one coalesced 128-byte load per
// line), counts the matches of all six symbols below each bound in its 32 positions (at most 32 each: twelve byte-wide partial
// counts in three dwords, summed over the group with DPP), and lane c < 6 forms count(c . q) from its own chunk's header word
// (A[c], bits 0..31) and the high byte that chunk 6 or 7 holds.  The six counts leave as one 48-byte row.
// Run blocks (run_index.hpp) rank each symbol with the format-aware constrain_any of k_constrain_ranges: correct, not tuned.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "plane_index.hpp"
#include "rank_ops.hpp"
#include "search_common.hpp"

namespace msbwt {
namespace {

// the positions of a plane-block chunk whose symbol is c
__device__ __forceinline__ uint32_t symbol_mask(const uint4 chunk, uint32_t c) {
    const uint32_t x0 = (c & 1u) ? 0u : ~0u, x1 = (c & 2u) ? 0u : ~0u, x2 = (c & 4u) ? 0u : ~0u;
    return (chunk.x ^ x0) & (chunk.y ^ x1) & (chunk.z ^ x2);
}

// rows: n x 6 u64; row q's words 0, 1 hold the range of query q on entry (launch_kmer_ranges, stride 6) and the six counts on exit
__global__ __launch_bounds__(256) void k_kmer_extensions(const uint4 *__restrict__ blocks, uint32_t format, const uint4 *__restrict__ overflow,
                                                         uint64_t total, uint64_t n, uint64_t *__restrict__ rows, uint32_t *__restrict__ flags) {
    const uint32_t sub = threadIdx.x & (kGroup - 1);
    const uint32_t group_base = (threadIdx.x & 63u) & ~uint32_t(kGroup - 1);
    const uint64_t ngroups = (uint64_t(gridDim.x) * blockDim.x) / kGroup;
    for (uint64_t q = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup; q < n; q += ngroups) {
        uint64_t *row = rows + q * 6u;
        const uint64_t l = row[0], h = row[1];  // (every lane of the group; lanes 0, 1 overwrite them below, after the loads)
        uint64_t mine = 0;                      // lane c < 6: count(c . q)
        if (l == ~0ull && h == ~0ull) {         // the query holds a code >= 6 (the search raised kFlagInvalidSymbol)
            mine = ~0ull;
        } else if (h > total || l > h) {        // never produced by the search: no wild line address from it
            mine = ~0ull;
            if (sub == 0u) atomicOr(flags, kFlagInternal);
        } else if (l != h) {                    // (an empty range touches no line: six zeros)
            if (format == uint32_t(kBlocksPlanes)) {
                const uint64_t bl = l >> kBlockShift, bh = h >> kBlockShift;
                const uint4 cl = blocks[bl * kGroup + sub];
                uint4 ch = cl;
                if (bh != bl) ch = blocks[bh * kGroup + sub];  // group-uniform
                const uint32_t ml = low_bits(min(max(int(uint32_t(l) & 255u) - int(sub * 32u), 0), 32));
                const uint32_t mh = low_bits(min(max(int(uint32_t(h) & 255u) - int(sub * 32u), 0), 32));
                // partial count i (i = c: below l, i = 6 + c: below h) in byte i & 3 of d[i >> 2]; each group total is at most 255
                uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
                for (uint32_t c = 0; c < 6u; ++c) {
                    d[c >> 2] |= uint32_t(__popc(symbol_mask(cl, c) & ml)) << ((c & 3u) * 8u);
                    d[(c + 6u) >> 2] |= uint32_t(__popc(symbol_mask(ch, c) & mh)) << (((c + 6u) & 3u) * 8u);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) d[i] = group_sum(d[i]);
                const uint32_t il = sub, ih = sub + 6u;  // (lanes 6, 7 compute nothing they keep)
                const uint32_t cnt_l = ((il < 4u ? d[0] : d[1]) >> ((il & 3u) * 8u)) & 0xFFu;
                const uint32_t cnt_h = ((ih < 8u ? d[1] : d[2]) >> ((ih & 3u) * 8u)) & 0xFFu;
                // A[c]: low word in chunk c's meta word (this lane's own), high byte in chunk 6 (c < 4) or 7 (c = 4, 5)
                const int hi_lane = int(group_base + 6u + ((sub >> 2) & 1u));
                const uint32_t sh = (sub & 3u) * 8u;
                const uint32_t hi_l = (uint32_t(__shfl(int(cl.w), hi_lane)) >> sh) & 0xFFu;
                const uint32_t hi_h = (uint32_t(__shfl(int(ch.w), hi_lane)) >> sh) & 0xFFu;
                const uint64_t bound_l = ((uint64_t(hi_l) << 32) | cl.w) + cnt_l;
                const uint64_t bound_h = ((uint64_t(hi_h) << 32) | ch.w) + cnt_h;
                mine = bound_h - bound_l;
            } else {
#pragma unroll 1
                for (uint32_t c = 0; c < 6u; ++c) {
                    const Range r = constrain_any(format, blocks, overflow, c, l, h, sub);
                    if (sub == c) mine = r.h - r.l;
                }
            }
        }
        if (sub < 6u) row[sub] = mine;
    }
}

}  // namespace

hipError_t launch_kmer_extensions(const IndexView &ix, uint64_t *rows, uint64_t n, uint32_t *flags, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_kmer_extensions, dim3(grid_for(n * kGroup)), dim3(256), 0, stream, static_cast<const uint4 *>(ix.blocks),
                       uint32_t(ix.block_format), static_cast<const uint4 *>(ix.overflow), ix.total, n, rows, flags);
    return hipGetLastError();
}

}  // namespace msbwt
