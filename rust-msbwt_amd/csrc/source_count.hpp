// Device-side counting over the source vector of a merged index (source_index.hpp), shared by k_range_sources (source_index.hip) and
// the by-source k-mer sink (source_spectrum.hip): the rows of one source in a range [l, h), by a kGroup-lane group per range.
//     narrow   h - l <= kSourceNarrow: lane j loads chunks j and j + 8 of the 256 bytes from l's 16-byte chunk on, bytes outside [l, h)
//              are overwritten with 0xFF, and four sources' counts travel in the bytes of one dword through one group sum
//     wide     rank(h) - rank(l): each bound its checkpoint plus the bytes from its block's start, at most 64 chunks
// Per-source counters never sit in an array indexed at run time (that would live in scratch memory).
// Include from HIP translation units only (the names are per translation unit, as in rank_ops.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rank_ops.hpp"
#include "source_index.hpp"

namespace msbwt {
namespace {

static_assert(kSourceNarrow + 15 <= 2 * kGroup * 16 && kSourceNarrow <= 255, "a narrow range lies in two chunks per lane and its counts in a byte");

__device__ __forceinline__ uint32_t low_bytes(int n) {  // the n lowest bytes of a dword, n clamped to 0..4
    n = min(max(n, 0), 4);
    return n >= 4 ? ~0u : ((1u << (8 * n)) - 1u);
}

// the 16-byte chunk at byte p of the vector with every byte outside [l, h) made 0xFF, which equals no source
__device__ __forceinline__ uint4 only_rows(uint4 c, uint64_t p, uint64_t l, uint64_t h) {
    const int lo = l > p ? int(min(l - p, uint64_t(16))) : 0, hi = h > p ? int(min(h - p, uint64_t(16))) : 0;  // bytes lo .. hi - 1 of the chunk stay
    return make_uint4(c.x | ~(low_bytes(hi) & ~low_bytes(lo)), c.y | ~(low_bytes(hi - 4) & ~low_bytes(lo - 4)),
                      c.z | ~(low_bytes(hi - 8) & ~low_bytes(lo - 8)), c.w | ~(low_bytes(hi - 12) & ~low_bytes(lo - 12)));
}

// bytes of w equal to the byte s4 repeats (exact for any bytes: no borrow or carry crosses a byte)
__device__ __forceinline__ uint32_t equal_bytes(uint32_t w, uint32_t s4) {
    const uint32_t x = w ^ s4;
    return uint32_t(__popc(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu)));
}
__device__ __forceinline__ uint32_t equal_bytes(uint4 c, uint32_t s4) {
    return equal_bytes(c.x, s4) + equal_bytes(c.y, s4) + equal_bytes(c.z, s4) + equal_bytes(c.w, s4);
}

// this lane's share of the rows of source s4 in [from, to), `from` a multiple of 16 and to - from <= kSourceBlockRows
__device__ __forceinline__ uint32_t span_count(const uint4 *__restrict__ rows16, uint64_t from, uint64_t to, uint32_t s4, uint32_t sub) {
    uint32_t cnt = 0;
#pragma unroll 1
    for (uint64_t p = from + sub * 16u; p < to; p += kGroup * 16u) cnt += equal_bytes(only_rows(rows16[p >> 4], p, from, to), s4);
    return cnt;
}

// ---- narrow: this lane's two chunks of a range of at most kSourceNarrow rows ----
struct NarrowRows {
    uint4 c0, c1;
};
__device__ __forceinline__ NarrowRows narrow_rows(const uint4 *__restrict__ rows16, uint64_t l, uint64_t h, uint32_t sub) {
    const uint64_t p0 = (l & ~15ull) + sub * 16u, p1 = p0 + kGroup * 16u;
    NarrowRows r{make_uint4(~0u, ~0u, ~0u, ~0u), make_uint4(~0u, ~0u, ~0u, ~0u)};
    if (p0 < h) r.c0 = only_rows(rows16[p0 >> 4], p0, l, h);
    if (p1 < h) r.c1 = only_rows(rows16[p1 >> 4], p1, l, h);
    return r;
}
// the counts of sources s0 .. s0 + 3 in the four bytes of one dword, summed over the group (every lane gets them)
__device__ __forceinline__ uint32_t narrow_four(const NarrowRows &r, uint32_t s0) {
    uint32_t packed = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t s4 = (s0 + j) * 0x01010101u;
        packed |= (equal_bytes(r.c0, s4) + equal_bytes(r.c1, s4)) << (8u * j);
    }
    return group_sum(packed);
}

// ---- wide: rank_s(h) - rank_s(l) from the two checkpoints and the bytes from each bound's block start (every lane gets it) ----
__device__ __forceinline__ uint64_t wide_count(const uint4 *__restrict__ rows16, const uint64_t *__restrict__ checkpoints, uint32_t stride, uint64_t l, uint64_t h,
                                               uint32_t s, uint32_t sub) {
    const uint64_t bl = l >> kSourceBlockShift, bh = h >> kSourceBlockShift;
    const uint32_t s4 = s * 0x01010101u;
    const uint32_t part = span_count(rows16, bh << kSourceBlockShift, h, s4, sub) - span_count(rows16, bl << kSourceBlockShift, l, s4, sub);
    return checkpoints[bh * stride + s] - checkpoints[bl * stride + s] + uint64_t(int64_t(int32_t(group_sum(part))));
}

}  // namespace
}  // namespace msbwt
