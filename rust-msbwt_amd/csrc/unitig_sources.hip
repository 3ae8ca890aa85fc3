// gfx950 (MI355X, CDNA4): the by-source sums of the unitig graph calls (unitig_sources.hpp) behind the emission of unitigs.hip.
//
// One kGroup-lane group per slot, as k_source_sink has one per staged k-mer.  All eight lanes read the slot's range, its state and the
// head's number (the same addresses: one request a group); in the canonical call, where the head is not emitted, all eight run the
// binary search for the mirror's slot in step.  The counts c_s come from the source vector alone (source_count.hpp): from the range's
// own bytes when it has at most kSourceNarrow rows, else from the two checkpoints plus the block prefixes.  Either way lane `sub` ends
// up holding the sources sub, sub + 8, sub + 16 and sub + 24 in four registers (a fully unrolled loop over the four batches of eight:
// never an array indexed at run time) and adds the non-zero ones to its unitig's row, so the adds of a group fall into one run of
// S consecutive words.
// Traffic per slot: 8 or 16 bytes of range, the 16-byte state and the head's 16 bytes, the 16-byte chunks the range touches (or two
// checkpoint lines and up to 2 KB of block prefix for a wide one), and one 64-bit atomic per source that holds the node.  Every word of
// sums is only ever added to, and integer sums commute: results do not depend on timing.  No MFMA.
#include <hip/hip_runtime.h>

#include "canonical.hpp"
#include "kernels.hpp"
#include "slot_bytes.hpp"
#include "source_count.hpp"
#include "unitig_slots.hpp"
#include "unitig_sources.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPerBlock = uint32_t(kThreads) / uint32_t(kGroup);
constexpr uint32_t kBatches = kSourceMax / uint32_t(kGroup);
static_assert(kSourceMax % kGroup == 0 && kBatches == 4, "lane sub holds sources sub, sub + 8, sub + 16, sub + 24");

template <bool kCanonical>
__global__ __launch_bounds__(kThreads) void k_unitig_source_sums(UnitigNodes g, const UnitigState *__restrict__ state, const UnitigState *__restrict__ heads, uint32_t k,
                                                                uint32_t probes, uint64_t U, UnitigSourceRanges ranges, const uint4 *__restrict__ rows16,
                                                                const uint64_t *__restrict__ checkpoints, uint64_t total, uint32_t n_sources, uint32_t stride,
                                                                unsigned long long *__restrict__ sums) {
    const uint32_t sub = threadIdx.x & uint32_t(kGroup - 1), group = threadIdx.x / uint32_t(kGroup);
    for (uint64_t base = uint64_t(blockIdx.x) * kPerBlock; base < ranges.m; base += uint64_t(gridDim.x) * kPerBlock) {  // (the same trips for the whole workgroup)
        const uint64_t j = base + group, i = ranges.first + j;
        const bool mine_slot = j < ranges.m && i < g.n;
        uint64_t l = 0, h = 0, u = U;
        bool broken = j < ranges.m && i >= g.n;  // (the host hands over slots only)
        if (mine_slot) {
            if (ranges.pairs) {
                l = ranges.pairs[2 * j];
                h = ranges.pairs[2 * j + 1];
            } else {
                l = ranges.l[i];
                h = l + g.counts[i];
            }
            if (l > h || h > total) broken = true;  // (a search and a walk return nothing else: no address is formed from another range)
            uint64_t head = head_of(g, state, i);
            if constexpr (kCanonical) {
                if (head < g.n && (byte_of(g.link_words, head) & kUnitigSkip)) {  // the mirror's unitig is the emitted one of the pair
                    const uint64_t mirror = slot_of(g.kmers, g.n, probes, reverse_complement_2bit(g.kmers[i], k));
                    head = mirror < g.n ? head_of(g, state, mirror) : g.n;
                    if (head < g.n && (byte_of(g.link_words, head) & kUnitigSkip)) head = g.n;
                }
            }
            if (head >= g.n) {
                broken = true;
            } else {
                u = heads[head].y;
                if (u >= U) broken = true;
            }
        }
        if (broken && sub == 0u) atomicOr(g.flags, kFlagInternal);
        const bool live = mine_slot && !broken && l < h;  // (the same in the whole group)
        const uint64_t width = h - l;
        uint64_t mine[kBatches] = {0, 0, 0, 0};
        if (live && width <= kSourceNarrow) {
            const NarrowRows r = narrow_rows(rows16, l, h, sub);
#pragma unroll
            for (uint32_t b = 0; b < kBatches; ++b) {
                if (b * kGroup < n_sources) {  // (the same branch in the whole group)
                    const uint32_t lo4 = narrow_four(r, b * kGroup), hi4 = b * kGroup + 4u < n_sources ? narrow_four(r, b * kGroup + 4u) : 0u;
                    mine[b] = ((sub < 4u ? lo4 : hi4) >> (8u * (sub & 3u))) & 0xFFu;
                }
            }
        } else if (live) {
#pragma unroll
            for (uint32_t b = 0; b < kBatches; ++b) {
#pragma unroll 1
                for (uint32_t t = 0; t < uint32_t(kGroup) && b * kGroup + t < n_sources; ++t) {
                    const uint64_t count = wide_count(rows16, checkpoints, stride, l, h, b * kGroup + t, sub);
                    if (sub == t) mine[b] = count;
                }
            }
        }
        if (live) {
            unsigned long long *row = sums + u * n_sources;  // (u < U: a row of the matrix)
#pragma unroll
            for (uint32_t b = 0; b < kBatches; ++b)
                if (mine[b] != 0ull && b * kGroup + sub < n_sources) atomicAdd(row + b * kGroup + sub, (unsigned long long)mine[b]);
        }
    }
}

}  // namespace

hipError_t launch_unitig_source_sums(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, bool canonical, uint32_t probes, uint64_t U,
                                     const SourceView &view, const UnitigSourceRanges &ranges, uint64_t *sums, hipStream_t stream) {
    const bool sources = view.rows && view.checkpoints && view.n_sources >= 1 && view.n_sources <= kSourceMax && view.stride >= view.n_sources;
    if (!g.kmers || !g.counts || !g.link_words || !g.flags || !state || !heads || !sources || !sums || k < 1 || k > (canonical ? 31u : 32u)) return hipErrorInvalidValue;
    if ((ranges.l == nullptr) == (ranges.pairs == nullptr) || ranges.first > g.n || ranges.m > g.n - ranges.first) return hipErrorInvalidValue;
    if (ranges.m == 0 || U == 0) return hipSuccess;
    const dim3 grid(capped_grid(ranges.m, kPerBlock, 256u * 8u));
    const uint4 *rows16 = reinterpret_cast<const uint4 *>(view.rows);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(sums);
    if (canonical)
        hipLaunchKernelGGL(k_unitig_source_sums<true>, grid, dim3(kThreads), 0, stream, g, state, heads, k, probes, U, ranges, rows16, view.checkpoints, view.total,
                           view.n_sources, view.stride, out);
    else
        hipLaunchKernelGGL(k_unitig_source_sums<false>, grid, dim3(kThreads), 0, stream, g, state, heads, k, probes, U, ranges, rows16, view.checkpoints, view.total,
                           view.n_sources, view.stride, out);
    return hipGetLastError();
}

}  // namespace msbwt
