// Left walks on the device: the kernels left_walk.hpp describes.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "left_walk.hpp"
#include "rank_ops.hpp"

namespace msbwt {
namespace {

// the symbol at a position and where LF takes it: C[s] + rank(s, position)
struct LfStep {
    uint32_t s;
    uint64_t next;
};

// Siblings of rank_ops.hpp's constrain and rank_runs_group that also return the symbol.  Called by all 8 lanes of a group with the
// same position; `sub` = lane index in the group, `group_base` = the wave lane of its first lane.

// `c`: this lane's chunk of the plane block that holds the position, `off` = position & 255
__device__ __forceinline__ LfStep lf_planes_line(const uint4 c, uint32_t off, uint32_t sub, uint32_t group_base) {
    const uint32_t bit = off & 31u;
    const uint32_t mine = ((c.x >> bit) & 1u) | (((c.y >> bit) & 1u) << 1) | (((c.z >> bit) & 1u) << 2);
    const uint32_t s = uint32_t(__shfl(int(mine), int(group_base + (off >> 5))));
    const uint32_t x0 = (s & 1u) ? 0u : ~0u, x1 = (s & 2u) ? 0u : ~0u, x2 = (s & 4u) ? 0u : ~0u;
    const int n = min(max(int(off) - int(sub * 32u), 0), 32);
    const uint32_t cnt = __popc((c.x ^ x0) & (c.y ^ x1) & (c.z ^ x2) & low_bits(n));  // <= 32, sum <= 255
    // the block's 40-bit bound A[s]: low word in chunk s, high byte in chunk 6 (s < 4) or 7
    const uint32_t lo = (sub == s) ? c.w : 0u;
    const uint32_t hi = (sub == 6u + (s >> 2)) ? ((c.w >> ((s & 3u) * 8u)) & 0xFFu) : 0u;
    const uint32_t packed = group_sum(cnt | (hi << 16));
    const uint32_t base = group_sum(lo);
    LfStep out;
    out.s = s;
    out.next = ((uint64_t(packed >> 16) << 32) | base) + (packed & 0xFFFFu);
    return out;
}

// `c`: this lane's chunk of the run block that holds the position, `off` = position & 511.  An OVERFLOW block: one more line, of the
// side array.  A block none of whose runs covers the offset (never on a well-formed index): next = all-ones.
__device__ __forceinline__ LfStep lf_runs_line(const uint4 c, const uint4 *__restrict__ overflow, uint32_t off, uint32_t sub, uint32_t group_base) {
    const uint32_t hi03 = uint32_t(__shfl(int(c.z), int(group_base + 1))), hi45 = uint32_t(__shfl(int(c.w), int(group_base + 1)));
    if (hi45 & kRunOverflowFlag) {  // group-uniform: two plane blocks, each with its own header
        const uint4 *two = overflow + uint64_t(uint32_t(__shfl(int(c.x), int(group_base + 2)))) * 16;
        return lf_planes_line(two[(off >> 8) * 8u + sub], off & 255u, sub, group_base);
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
    const int first = int(inc - mine), r = int(off);
    uint32_t found = 0;  // 8 | symbol of the run that covers the offset: one run of one lane
    if (sub >= 2u) {
        int cur = first;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t run = (word[j] >> (8 * b)) & 0xFFu;
                const int len = int(run >> 3);
                if (r >= cur && r < cur + len) found = 8u | (run & 7u);
                cur += len;
            }
        }
    }
    found = group_sum(found);
    const uint32_t s = found & 7u;
    uint32_t cnt = 0;  // matches before the offset (<= 512)
    if (sub >= 2u) {
        int cur = first;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t run = (word[j] >> (8 * b)) & 0xFFu;
                const int len = int(run >> 3);
                if ((run & 7u) == s) cnt += uint32_t(min(max(r - cur, 0), len));
                cur += len;
            }
        }
    }
    cnt = group_sum(cnt);
    // header: A[s] low word in word s (lane s >> 2, component s & 3), high byte in word 6 / 7 (lane 1)
    const uint32_t w0 = uint32_t(__shfl(int(s == 0u ? c.x : s == 1u ? c.y : s == 2u ? c.z : c.w), int(group_base)));
    const uint32_t w1 = uint32_t(__shfl(int(s == 4u ? c.x : c.y), int(group_base + 1)));
    const uint32_t lo = (s & 4u) ? w1 : w0;
    const uint32_t hi = (((s >> 2) ? hi45 : hi03) >> ((s & 3u) * 8u)) & 0xFFu;
    LfStep out;
    out.s = s;
    out.next = (found >> 3) == 1u ? ((uint64_t(hi) << 32) | lo) + cnt : ~0ull;
    return out;
}

// the bytes of `acc` (`cnt` of them, 1..8, the first at p) stored: one 8-byte word where there are eight -- p is aligned then --,
// else a byte a lane
__device__ __forceinline__ void store_symbols(uint8_t *p, uint64_t acc, uint32_t cnt, uint32_t sub) {
    if (cnt == 8u) {
        if (sub == 0u) *reinterpret_cast<uint64_t *>(p) = acc;
    } else if (sub < cnt) {
        p[sub] = uint8_t(acc >> (8u * sub));
    }
}

template <uint32_t kFormat>
__global__ __launch_bounds__(256) void k_left_walk(const LeftWalkCall c) {
    constexpr uint32_t W = kLeftWalkSlots;
    constexpr uint32_t kLive = 0u, kNoWalk = 0xFFu;
    __shared__ unsigned long long tally[kWalkCounterWords];
    if (threadIdx.x < kWalkCounterWords) tally[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t sub = threadIdx.x & (kGroup - 1), group_base = (threadIdx.x & 63u) & ~7u;
    const uint64_t g = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const uint4 *__restrict__ blocks = static_cast<const uint4 *>(c.blocks);
    const uint4 *__restrict__ overflow = static_cast<const uint4 *>(c.overflow);
    constexpr uint32_t kShift = kFormat == 0u ? 8u : 9u;  // positions a block: 256 (planes), 512 (runs)

    uint64_t row[W], steps[W], acc[W], read[W];
    uint32_t cnt[W], stop[W];
    uint8_t *out[W];
#pragma unroll
    for (uint32_t u = 0; u < W; ++u) {
        const uint64_t i = g * W + u;
        row[u] = steps[u] = acc[u] = 0;
        read[u] = ~0ull;
        cnt[u] = 0;
        stop[u] = kNoWalk;
        out[u] = nullptr;
        if (i < c.n) {
            row[u] = c.rows ? c.rows[i] : c.first_row + i;
            const bool bad = row[u] >= c.total || (c.ids && row[u] >= c.dollars);
            stop[u] = bad ? uint32_t(kWalkBadRow) : kLive;
            if (bad && sub == 0u) atomicOr(c.flags, kFlagInvalidRange);
            if (c.symbols) out[u] = c.symbols + i * c.stride;
        }
    }

    // t = max_steps fetches a line only to tell DOLLAR from MAX_STEPS; nothing is emitted there
    for (uint64_t t = 0; t <= c.max_steps; ++t) {
        uint4 line[W];
        bool any = false;
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            line[u] = uint4{0u, 0u, 0u, 0u};
            if (stop[u] == kLive) {  // row < total: inside the block array
                line[u] = blocks[(row[u] >> kShift) * kGroup + sub];
                any = true;
            }
        }
        if (!any) break;  // (group-uniform)
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            if (stop[u] != kLive) continue;
            const uint32_t off = uint32_t(row[u]) & ((1u << kShift) - 1u);
            const LfStep st = kFormat == 0u ? lf_planes_line(line[u], off, sub, group_base) : lf_runs_line(line[u], overflow, off, sub, group_base);
            if (st.s == 0u) {  // '$': neither emitted nor counted; C['$'] = 0, so LF is the read
                stop[u] = kWalkDollar;
                read[u] = st.next;
            } else if (t == c.max_steps) {
                stop[u] = kWalkMaxSteps;
            } else if (st.next >= c.total) {  // never on a well-formed index: no address is formed from it
                if (sub == 0u) atomicOr(c.flags, kFlagInternal);
                stop[u] = kWalkBadRow;
            } else {
                row[u] = st.next;
                ++steps[u];
                if (out[u]) {
                    acc[u] |= uint64_t(st.s) << (8u * cnt[u]);
                    ++cnt[u];
                    uint8_t *end = out[u] + steps[u];
                    if ((reinterpret_cast<uintptr_t>(end) & 7u) == 0u) {  // the bytes held end on a word border
                        store_symbols(end - cnt[u], acc[u], cnt[u], sub);
                        acc[u] = 0;
                        cnt[u] = 0;
                    }
                }
            }
            if (stop[u] != kLive && cnt[u]) store_symbols(out[u] + steps[u] - cnt[u], acc[u], cnt[u], sub);  // the ragged end
        }
    }

    if (sub == 0u) {
        unsigned long long sum = 0, stops[3] = {0, 0, 0};
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            const uint64_t i = g * W + u;
            if (stop[u] == kNoWalk) continue;
            if (c.steps) c.steps[i] = steps[u];
            if (c.stops) c.stops[i] = uint8_t(stop[u]);
            if (c.last) c.last[i] = row[u];
            if (c.reads) c.reads[i] = read[u];
            sum += steps[u];
            if (stop[u] >= kWalkDollar && stop[u] <= kWalkBadRow) ++stops[stop[u] - kWalkDollar];
        }
        if (sum) atomicAdd(&tally[kWalkSteps], sum);
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j)
            if (stops[j]) atomicAdd(&tally[kWalkDollars + j], stops[j]);
    }
    __syncthreads();
    if (threadIdx.x < kWalkCounterWords && tally[threadIdx.x]) atomicAdd(c.counters + threadIdx.x, tally[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_left_walk_reverse(const uint8_t *__restrict__ rows, uint64_t stride, const uint64_t *__restrict__ offsets, uint64_t n, uint64_t base,
                                                           uint8_t *__restrict__ out, uint64_t room, uint64_t *__restrict__ out_offsets, uint32_t *flags) {
    const uint64_t j = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (j >= n) return;
    const uint64_t from = offsets[j], to = offsets[j + 1], len = to - from;
    if (out_offsets && lane == 0u) {
        out_offsets[j] = base + from;
        if (j + 1 == n) out_offsets[n] = base + to;
    }
    if (!out) return;
    if (to < from || len > stride || to > room) {
        if (lane == 0u) atomicOr(flags, kFlagInternal);
        return;
    }
    const uint8_t *src = rows + j * stride;
    for (uint64_t p = lane; p < len; p += 64) out[from + p] = src[len - 1 - p];  // len <= stride, which the host fixed
}

}  // namespace

hipError_t launch_left_walk(const LeftWalkCall &c, hipStream_t stream) {
    if (c.n == 0) return hipSuccess;
    if (c.n > kWalkMaxPiece || !c.counters || !c.flags || (c.total && !c.blocks)) return hipErrorInvalidValue;
    const uint64_t groups = (c.n + kLeftWalkSlots - 1) / kLeftWalkSlots;
    const dim3 grid(uint32_t((groups * kGroup + 255) / 256)), block(256);
    if (c.format == 0u)
        hipLaunchKernelGGL(k_left_walk<0u>, grid, block, 0, stream, c);
    else
        hipLaunchKernelGGL(k_left_walk<1u>, grid, block, 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_left_walk_reverse(const uint8_t *rows, uint64_t stride, const uint64_t *offsets, uint64_t n, uint64_t base, uint8_t *out_symbols, uint64_t room,
                                    uint64_t *out_offsets, uint32_t *flags, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kWalkMaxPiece || !offsets || (out_symbols && !rows)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_left_walk_reverse, dim3(uint32_t((n * 64 + 255) / 256)), dim3(256), 0, stream, rows, stride, offsets, n, base, out_symbols, room, out_offsets, flags);
    return hipGetLastError();
}

}  // namespace msbwt
