// Read overlaps on the device: the kernels overlaps.hpp describes.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "overlaps.hpp"
#include "rank_ops.hpp"

namespace msbwt {
namespace {

// A[s] + the occurrences of s before a position, and the same for '$' (code 0, whose C is 0: the reads before the position); `extra`:
// the side-array lines fetched for it.  Called by all 8 lanes of a group with the same position and symbol; `sub` = lane index in the
// group, `group_base` = the wave lane of its first lane.
struct Rank2 {
    uint64_t s, dollar;
    uint32_t extra;
};

// `c`: this lane's chunk of the plane block that holds the position, `off` = position & 255; s in 1..5
__device__ __forceinline__ Rank2 rank2_planes(const uint4 c, uint32_t off, uint32_t s, uint32_t sub) {
    const uint32_t x0 = (s & 1u) ? 0u : ~0u, x1 = (s & 2u) ? 0u : ~0u, x2 = (s & 4u) ? 0u : ~0u;
    const uint32_t mask = low_bits(min(max(int(off) - int(sub * 32u), 0), 32));
    const uint32_t cnt_s = __popc((c.x ^ x0) & (c.y ^ x1) & (c.z ^ x2) & mask);  // <= 32, sum <= 255
    const uint32_t cnt_d = __popc(~(c.x | c.y | c.z) & mask);
    // the block's 40-bit bounds: low word of A[s] in chunk s, high byte in chunk 6 (s < 4) or 7
    const uint32_t lo_s = (sub == s) ? c.w : 0u, lo_d = (sub == 0u) ? c.w : 0u;
    const uint32_t hi_s = (sub == 6u + (s >> 2)) ? ((c.w >> ((s & 3u) * 8u)) & 0xFFu) : 0u;
    const uint32_t hi_d = (sub == 6u) ? (c.w & 0xFFu) : 0u;
    // four byte-wide fields never carry into each other: counts sum to <= 255, one lane owns each high byte
    const uint32_t packed = group_sum(cnt_s | (hi_s << 8) | (cnt_d << 16) | (hi_d << 24));
    const uint32_t base_s = group_sum(lo_s), base_d = group_sum(lo_d);
    Rank2 out;
    out.s = ((uint64_t((packed >> 8) & 0xFFu) << 32) | base_s) + (packed & 0xFFu);
    out.dollar = ((uint64_t(packed >> 24) << 32) | base_d) + ((packed >> 16) & 0xFFu);
    out.extra = 0u;
    return out;
}

// `c`: this lane's chunk of the run block that holds the position, `off` = position & 511.  An OVERFLOW block: one more line, of the
// side array, plane-shaped with its own header.
__device__ __forceinline__ Rank2 rank2_runs(const uint4 c, const uint4 *__restrict__ overflow, uint32_t off, uint32_t s, uint32_t sub, uint32_t group_base) {
    const uint32_t hi03 = uint32_t(__shfl(int(c.z), int(group_base + 1))), hi45 = uint32_t(__shfl(int(c.w), int(group_base + 1)));
    if (hi45 & kRunOverflowFlag) {  // group-uniform
        const uint4 *two = overflow + uint64_t(uint32_t(__shfl(int(c.x), int(group_base + 2)))) * 16;
        Rank2 out = rank2_planes(two[(off >> 8) * 8u + sub], off & 255u, s, sub);
        out.extra = 1u;
        return out;
    }
    const uint32_t word[4] = {c.x, c.y, c.z, c.w};
    uint32_t mine = 0;  // symbols my 16 runs cover (lanes 0,1: none)
    if (sub >= 2u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mine = __builtin_amdgcn_sad_u8((word[j] >> 3) & 0x1F1F1F1Fu, 0u, mine);
    }
    uint32_t inc = mine;  // inclusive prefix over the 8 lanes
    for (int d = 1; d < 8; d <<= 1) {
        const uint32_t y = uint32_t(__shfl_up(int(inc), d, 8));
        if (int(sub) >= d) inc += y;
    }
    const int r = int(off);
    uint32_t cnt = 0;  // matches of s before the offset in the low half, of '$' in the high half (each <= 512)
    if (sub >= 2u) {
        int cur = int(inc - mine);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t run = (word[j] >> (8 * b)) & 0xFFu;
                const int len = int(run >> 3);
                const uint32_t clipped = uint32_t(min(max(r - cur, 0), len));
                if ((run & 7u) == s) cnt += clipped;
                if ((run & 7u) == 0u) cnt += clipped << 16;
                cur += len;
            }
        }
    }
    cnt = group_sum(cnt);
    // header: A[s] low word in word s (lane s >> 2, component s & 3), high byte in word 6 / 7 (lane 1)
    const uint32_t w0 = uint32_t(__shfl(int(s == 1u ? c.y : s == 2u ? c.z : c.w), int(group_base)));
    const uint32_t w1 = uint32_t(__shfl(int(s == 4u ? c.x : c.y), int(group_base + 1)));
    const uint32_t lo_s = (s & 4u) ? w1 : w0, lo_d = uint32_t(__shfl(int(c.x), int(group_base)));
    const uint32_t hi_s = (((s >> 2) ? hi45 : hi03) >> ((s & 3u) * 8u)) & 0xFFu;
    Rank2 out;
    out.s = ((uint64_t(hi_s) << 32) | lo_s) + (cnt & 0xFFFFu);
    out.dollar = ((uint64_t(hi03 & 0xFFu) << 32) | lo_d) + (cnt >> 16);
    out.extra = 0u;
    return out;
}

// COMPLEMENT_INT = [0, 5, 3, 2, 4, 1] as nibbles; a code above 5 stays what it is
__device__ __forceinline__ uint32_t complement(uint32_t s) { return s < 6u ? (0x142350u >> (4u * s)) & 0xFu : s; }

// The next symbol of the string searched.  Strand 0: the query's symbols [lim, pos) from the end backwards; strand 1: [pos, lim) from
// the start forwards, complemented.  At least one symbol is left.  `buf` holds `have` symbols read ahead: eight where an aligned word
// lies inside what is left, else one.
__device__ __forceinline__ uint32_t next_symbol(const uint8_t *__restrict__ symbols, uint64_t &pos, uint64_t lim, uint64_t &buf, uint32_t &have, uint32_t strand) {
    const uint8_t *a = symbols + pos;
    const bool aligned = (reinterpret_cast<uintptr_t>(a) & 7u) == 0u;
    uint32_t s;
    if (strand == 0u) {
        if (have == 0u) {
            if (aligned && pos - lim >= 8u) {
                buf = *reinterpret_cast<const uint64_t *>(a - 8);
                have = 8u;
            } else {
                buf = uint64_t(a[-1]) << 56;
                have = 1u;
            }
        }
        s = uint32_t(buf >> 56);
        buf <<= 8;
        --pos;
    } else {
        if (have == 0u) {
            if (aligned && lim - pos >= 8u) {
                buf = *reinterpret_cast<const uint64_t *>(a);
                have = 8u;
            } else {
                buf = uint64_t(a[0]);
                have = 1u;
            }
        }
        s = complement(uint32_t(buf & 0xFFu));
        buf >>= 8;
        ++pos;
    }
    --have;
    return s;
}

template <uint32_t kFormat>
__global__ __launch_bounds__(256) void k_overlaps(const OverlapCall c) {
    constexpr uint32_t W = kOverlapSlots;
    constexpr uint32_t kLive = 0u, kNoQuery = 0xFFu;
    __shared__ unsigned long long tally[kOverlapCounterWords];
    if (threadIdx.x < kOverlapCounterWords) tally[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t sub = threadIdx.x & (kGroup - 1), group_base = (threadIdx.x & 63u) & ~7u;
    const uint64_t g = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const uint4 *__restrict__ blocks = static_cast<const uint4 *>(c.blocks);
    const uint4 *__restrict__ overflow = static_cast<const uint4 *>(c.overflow);
    constexpr uint32_t kShift = kFormat == 0u ? 8u : 9u;  // positions a block: 256 (planes), 512 (runs)
    constexpr uint32_t kMask = (1u << kShift) - 1u;
    const bool fill = c.lengths != nullptr;

    uint64_t l[W], h[W], pos[W], lim[W], buf[W], E[W], matched[W], nrec[W], edges[W], out_at[W], room[W], lines[W];
    uint32_t have[W], stop[W];
#pragma unroll
    for (uint32_t u = 0; u < W; ++u) {
        const uint64_t i = g * W + u;
        l[u] = h[u] = pos[u] = lim[u] = buf[u] = E[u] = matched[u] = nrec[u] = edges[u] = out_at[u] = room[u] = lines[u] = 0;
        have[u] = 0;
        stop[u] = kNoQuery;
        if (i < c.n) {
            const uint64_t from = c.offsets[i], to = c.offsets[i + 1];
            uint64_t L = 0;
            if (to < from || from < c.origin) {
                if (sub == 0u) atomicOr(c.flags, kFlagInvalidRange);
            } else {
                L = to - from;
            }
            E[u] = (c.max_overlap && c.max_overlap < L) ? c.max_overlap : L;
            if (E[u] > c.trips) {  // never: the host fixed trips from these very offsets
                if (sub == 0u) atomicOr(c.flags, kFlagInternal);
                E[u] = c.trips;
            }
            const uint64_t rel = L ? from - c.origin : 0;  // (an empty query reads nothing)
            pos[u] = c.strand == 0u ? rel + L : rel;
            lim[u] = c.strand == 0u ? rel : rel + L;
            stop[u] = kLive;
            if (fill) {
                const uint64_t a = c.rec_offsets[i], b = c.rec_offsets[i + 1];
                out_at[u] = c.base + a;
                room[u] = b >= a ? b - a : 0;
            }
        }
    }

    // every live query stands at j = t
    for (uint64_t t = 0; t <= c.trips; ++t) {
        uint4 line_l[W], line_h[W];
        uint32_t sym[W];
        bool any = false;
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            line_l[u] = line_h[u] = uint4{0u, 0u, 0u, 0u};
            sym[u] = 0u;
            if (stop[u] != kLive) continue;
            if (t == E[u] && (t == 0 || t < c.min_overlap)) {  // nothing to emit, nothing to fetch
                stop[u] = kOverlapEnd;
                matched[u] = t;
                continue;
            }
            any = true;
            if (t < E[u]) sym[u] = next_symbol(c.symbols, pos[u], lim[u], buf[u], have[u], c.strand);
            if (t == 0) continue;
            // l < h <= total: l is inside the block array, h where it is below total
            line_l[u] = blocks[(l[u] >> kShift) * kGroup + sub];
            if (h[u] < c.total && (h[u] >> kShift) != (l[u] >> kShift)) line_h[u] = blocks[(h[u] >> kShift) * kGroup + sub];
        }
        if (!any) break;  // (group-uniform)
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            if (stop[u] != kLive) continue;
            const uint32_t s = sym[u];
            const bool good = s >= 1u && s <= 5u;
            uint64_t nl, nh;
            if (t == 0) {  // R_1 from the symbol counts (E >= 1 here)
                nl = good ? c.start[s] : 0;
                nh = good ? c.start[s + 1] : 0;
            } else {
                const uint32_t rs = good ? s : 1u;
                const bool inside = h[u] < c.total, same = (h[u] >> kShift) == (l[u] >> kShift);
                const uint32_t off_l = uint32_t(l[u]) & kMask, off_h = uint32_t(h[u]) & kMask;
                Rank2 a, b;
                if (kFormat == 0u) {
                    a = rank2_planes(line_l[u], off_l, rs, sub);
                } else {
                    a = rank2_runs(line_l[u], overflow, off_l, rs, sub, group_base);
                }
                if (!inside) {  // rank(., T): the counts
                    b.s = c.start[rs + 1];
                    b.dollar = c.start[1];
                    b.extra = 0u;
                } else if (kFormat == 0u) {
                    b = rank2_planes(same ? line_l[u] : line_h[u], off_h, rs, sub);
                } else {
                    b = rank2_runs(same ? line_l[u] : line_h[u], overflow, off_h, rs, sub, group_base);
                }
                lines[u] += 1u + ((inside && !same) ? 1u : 0u) + a.extra + b.extra;
                if (t >= c.min_overlap && b.dollar > a.dollar) {  // the reads that begin with the last t symbols
                    const uint64_t k = nrec[u], count = b.dollar - a.dollar;
                    if (fill) {
                        const uint64_t at = out_at[u] + k;
                        if (k >= room[u] || at >= c.capacity) {  // never: pass A counted these records
                            if (sub == 0u) atomicOr(c.flags, kFlagInternal);
                        } else if (sub == (uint32_t(k) & 7u)) {
                            c.lengths[at] = t;
                            c.first[at] = a.dollar;
                            c.counts[at] = count;
                        }
                    }
                    nrec[u] = k + 1;
                    edges[u] += count;
                }
                if (t == E[u]) {
                    stop[u] = kOverlapEnd;
                    matched[u] = t;
                    continue;
                }
                nl = a.s;
                nh = b.s;
            }
            if (!good) {
                if (sub == 0u) atomicOr(c.flags, kFlagInvalidSymbol);
                stop[u] = kOverlapBadSymbol;
                matched[u] = t;
                continue;
            }
            if (nh > c.total) {  // never on a well-formed index: no address is formed from it
                if (sub == 0u) atomicOr(c.flags, kFlagInternal);
                nh = nl;
            }
            if (nl >= nh) {
                stop[u] = kOverlapEmpty;
                matched[u] = t;
                continue;
            }
            l[u] = nl;
            h[u] = nh;
        }
    }

    if (sub == 0u) {
        unsigned long long sums[kOverlapCounterWords] = {};
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            const uint64_t i = g * W + u;
            if (stop[u] == kNoQuery) continue;
            if (stop[u] == kLive) {  // never: every query stops at t == E <= trips
                atomicOr(c.flags, kFlagInternal);
                stop[u] = kOverlapEmpty;
            }
            sums[kOverlapLines] += lines[u];
            if (fill) continue;
            if (c.rec_counts) c.rec_counts[i] = nrec[u];
            if (c.matched) c.matched[i] = matched[u];
            if (c.edges) c.edges[i] = edges[u];
            if (c.stops) c.stops[i] = uint8_t(stop[u]);
            sums[kOverlapSymbols] += matched[u];
            sums[kOverlapRecords] += nrec[u];
            sums[kOverlapEdges] += edges[u];
            ++sums[kOverlapEnds + (stop[u] - kOverlapEnd)];
        }
#pragma unroll
        for (uint32_t j = 0; j < kOverlapMaxE; ++j)
            if (sums[j]) atomicAdd(&tally[j], sums[j]);
    }
    __syncthreads();
    if (threadIdx.x < kOverlapMaxE && tally[threadIdx.x]) atomicAdd(c.counters + threadIdx.x, tally[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_overlap_prepare(const uint64_t *__restrict__ offsets, uint64_t n, uint64_t max_overlap, unsigned long long *counters,
                                                         uint32_t *flags) {
    __shared__ unsigned long long most;
    if (threadIdx.x == 0) most = 0ull;
    __syncthreads();
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint64_t from = offsets[i], to = offsets[i + 1];
        if (to < from) {
            atomicOr(flags, kFlagInvalidRange);
        } else {
            const uint64_t L = to - from;
            const unsigned long long E = (max_overlap && max_overlap < L) ? max_overlap : L;
            if (E) atomicMax(&most, E);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && most) atomicMax(counters + kOverlapMaxE, most);
}

__global__ __launch_bounds__(256) void k_overlap_offsets(const uint64_t *__restrict__ scanned, uint64_t words, uint64_t base, uint64_t *__restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < words) out[i] = base + scanned[i];
}

}  // namespace

hipError_t launch_overlaps(const OverlapCall &c, hipStream_t stream) {
    if (c.n == 0) return hipSuccess;
    const bool some = c.lengths || c.first || c.counts, all = c.lengths && c.first && c.counts;
    if (c.n > kOverlapMaxPiece || !c.counters || !c.flags || !c.offsets || !c.symbols || !c.total || !c.blocks || c.min_overlap == 0 || c.strand > 1u || some != all ||
        (all && (!c.rec_offsets || c.rec_counts)))
        return hipErrorInvalidValue;
    const uint64_t groups = (c.n + kOverlapSlots - 1) / kOverlapSlots;
    const dim3 grid(uint32_t((groups * kGroup + 255) / 256)), block(256);
    if (c.format == 0u)
        hipLaunchKernelGGL(k_overlaps<0u>, grid, block, 0, stream, c);
    else
        hipLaunchKernelGGL(k_overlaps<1u>, grid, block, 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_overlap_prepare(const uint64_t *offsets, uint64_t n, uint64_t max_overlap, unsigned long long *counters, uint32_t *flags, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kOverlapMaxPiece || !offsets || !counters || !flags) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_overlap_prepare, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, offsets, n, max_overlap, counters, flags);
    return hipGetLastError();
}

hipError_t launch_overlap_offsets(const uint64_t *scanned, uint64_t words, uint64_t base, uint64_t *out, hipStream_t stream) {
    if (words == 0) return hipSuccess;
    if (words > kOverlapMaxPiece + 1 || !scanned || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_overlap_offsets, dim3(uint32_t((words + 255) / 256)), dim3(256), 0, stream, scanned, words, base, out);
    return hipGetLastError();
}

}  // namespace msbwt
