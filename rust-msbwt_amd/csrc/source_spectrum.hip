// gfx950 (MI355X, CDNA4): the sink of the by-source k-mer calls (source_spectrum.hpp) over the k-mers a chunk of the walk staged.
//
// One kGroup-lane group per staged k-mer {word, l, h}, as k_range_sources.  Its counts c_s come from the source vector alone
// (source_count.hpp): from the range's own bytes when h - l <= kSourceNarrow -- a present 31-mer at 30 x has some 30 rows -- else from the
// two checkpoints plus the block prefixes.  Either way lane `sub` of the group ends up holding the sources sub, sub + 8, sub + 16 and
// sub + 24 in four registers (a fully unrolled loop over the four batches of eight: never an array indexed at run time), and that is
// the only place a k-mer's counts ever are:
//     predicate   each lane judges its own sources against limits it loaded once per kernel; one group sum carries the failures and
//                 the number of sources that hold the k-mer to all eight lanes.  The sum of the counts is h - l: every row has a source.
//     histogram   fed from those registers: bin c_s of source s, the bins below kSourceLdsWords / source_stride(S) in LDS (16 KB at every
//                 S, flushed once per workgroup), wider ones by global atomics.  Absent sources (c_s = 0) tally nothing -- at 32 sources
//                 nearly every pair (k-mer, source) is one -- and bin 0 is what the caller derives: k-mers - distinct[s].  The sums of
//                 c_s stay in four more registers per lane until the workgroup ends; the sharing tallies (33 words) are LDS.
//     count/mark  how many k-mers pass (summed per thread, one atomic per workgroup); for a sorted dump the bit of each one's l (spectrum.hpp's rank view)
//     append      the passing records, wherever the workgroup's reservation puts them
//     scatter     the passing records, each at the rank of its l: ascending k-mers, no sort
// Only a record that passes is written: eight lanes store its S counts as 64-byte pieces, lane 0 its word and l.
// Traffic per k-mer: 24 bytes of the staged record, and the 16-byte chunks its range touches (or two checkpoint lines and up to 2 KB of
// block prefix for a wide one), random lines of an array that is far larger than the caches.  Integer work: no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "frontier.hpp"
#include "kernels.hpp"
#include "source_count.hpp"
#include "source_spectrum.hpp"
#include "spectrum.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = kFrontierThreads;  // (reserve and block_add are sized by it)
constexpr uint32_t kPerBlock = uint32_t(kThreads) / uint32_t(kGroup);
constexpr uint32_t kBatches = kSourceMax / uint32_t(kGroup);
static_assert(kSourceMax % kGroup == 0 && kBatches == 4, "lane sub holds sources sub, sub + 8, sub + 16, sub + 24");
static_assert(kSourceLdsWords % kSourceMax == 0, "every source gets the same whole number of LDS bins");

// the value lane 0 of this lane's group holds
__device__ __forceinline__ uint64_t group_first(uint64_t x) {
    const int src = int(threadIdx.x & 63u & ~uint32_t(kGroup - 1));
    const uint32_t lo = uint32_t(__shfl(int(uint32_t(x)), src)), hi = uint32_t(__shfl(int(uint32_t(x >> 32)), src));
    return (uint64_t(hi) << 32) | lo;
}

__global__ __launch_bounds__(kThreads) void k_source_sink(const Node *__restrict__ staged, uint64_t m, const uint4 *__restrict__ rows16,
                                                         const uint64_t *__restrict__ checkpoints, uint64_t total, uint32_t n_sources, uint32_t stride, SourceSink sink) {
    __shared__ uint32_t lds_hist[kSourceLdsWords];
    __shared__ unsigned long long lds_occ[kSourceMax];
    __shared__ uint32_t lds_share[kSourceMax + 1];
    const bool hist = sink.mode == kSourceSinkHist;
    const uint32_t lds_bins = kSourceLdsWords / stride;  // per source
    const uint32_t sub = threadIdx.x & uint32_t(kGroup - 1), group = threadIdx.x / uint32_t(kGroup);
    if (hist) {
        for (uint32_t b = threadIdx.x; b < kSourceLdsWords; b += kThreads) lds_hist[b] = 0u;
        if (threadIdx.x < kSourceMax) lds_occ[threadIdx.x] = 0ull;
        if (threadIdx.x <= kSourceMax) lds_share[threadIdx.x] = 0u;
        __syncthreads();
    }
    // this lane's sources are sub + 8 j: their limits, and (histogram) the sums of their counts
    uint64_t lo[kBatches], hi[kBatches], occ[kBatches];
#pragma unroll
    for (uint32_t j = 0; j < kBatches; ++j) {
        const uint32_t s = j * kGroup + sub;
        const bool real = s < n_sources && !hist;
        lo[j] = real ? sink.limits[s] : 0ull;
        hi[j] = real ? sink.limits[kSourceMax + s] : ~0ull;
        occ[j] = 0ull;
    }
    uint32_t passed = 0;  // count / mark: this thread's, summed once per workgroup (one word takes only so many atomics a microsecond)
    for (uint64_t base = uint64_t(blockIdx.x) * kPerBlock; base < m; base += uint64_t(gridDim.x) * kPerBlock) {  // (the same trips for the whole workgroup)
        const uint64_t i = base + group;
        Node nd{0, 0, 0};
        if (i < m) nd = staged[i];
        const uint64_t l = nd.l, h = nd.h, width = h - l;
        const bool live = i < m && l < h && h <= total;  // (the walk stages nothing else: no address is formed from another range)
        if (i < m && !live && sub == 0u) atomicOr(sink.flags, kFlagInternal);
        uint64_t mine[kBatches] = {0, 0, 0, 0};
        if (live && width <= kSourceNarrow) {
            const NarrowRows r = narrow_rows(rows16, l, h, sub);
#pragma unroll
            for (uint32_t j = 0; j < kBatches; ++j) {
                if (j * kGroup < n_sources) {  // (the same branch in the whole group)
                    const uint32_t a = narrow_four(r, j * kGroup), b = j * kGroup + 4u < n_sources ? narrow_four(r, j * kGroup + 4u) : 0u;
                    mine[j] = ((sub < 4u ? a : b) >> (8u * (sub & 3u))) & 0xFFu;
                }
            }
        } else if (live) {
#pragma unroll
            for (uint32_t j = 0; j < kBatches; ++j) {
#pragma unroll 1
                for (uint32_t t = 0; t < uint32_t(kGroup) && j * kGroup + t < n_sources; ++t) {
                    const uint64_t count = wide_count(rows16, checkpoints, stride, l, h, j * kGroup + t, sub);
                    if (sub == t) mine[j] = count;
                }
            }
        }
        // (a source >= n_sources has no rows: its count is 0 and its limits let 0 pass)
        uint32_t fails = 0, held = 0;
#pragma unroll
        for (uint32_t j = 0; j < kBatches; ++j) {
            const uint64_t c = mine[j];
            fails += (c < lo[j] || c > hi[j]) ? 1u : 0u;
            held += c != 0ull ? 1u : 0u;
            if (hist && c != 0ull) {
                const uint32_t s = j * kGroup + sub;
                const uint64_t bin = min(c, sink.n_bins - 1u);
                if (bin < lds_bins) atomicAdd(&lds_hist[s * lds_bins + uint32_t(bin)], 1u);
                else atomicAdd(sink.hist + uint64_t(s) * sink.n_bins + bin, 1ull);
                occ[j] += c;
            }
        }
        const uint32_t both = group_sum(fails | (held << 16));
        const bool pass = live && (both & 0xFFFFu) == 0u && width >= sink.min_total && width <= sink.max_total;
        const uint32_t one = pass && sub == 0u ? 1u : 0u;
        if (hist) {
            if (live && sub == 0u) atomicAdd(&lds_share[both >> 16], 1u);
        } else if (sink.mode == kSourceSinkCount) {
            passed += one;
            if (one && sink.bitmap) atomicOr(sink.bitmap + (l >> 5), 1u << (uint32_t(l) & 31u));
        } else {
            uint64_t place = 0;
            if (sink.mode == kSourceSinkAppend) place = reserve(one, sink.totals + kSourceOut);
            else if (one) place = spectrum_rank_below(sink.bitmap, sink.prefix, l);
            place = group_first(place);
            if (pass) {
                if (place < sink.capacity) {
                    if (sub == 0u) {
                        sink.kmers[place] = nd.key;
                        if (sink.l) sink.l[place] = l;
                    }
                    if (sink.counts) {
#pragma unroll
                        for (uint32_t j = 0; j < kBatches; ++j)
                            if (j * kGroup + sub < n_sources) sink.counts[place * n_sources + j * kGroup + sub] = mine[j];
                    }
                } else if (sub == 0u) {
                    atomicOr(sink.flags, kFlagInternal);
                }
            }
        }
    }
    if (sink.mode == kSourceSinkCount) block_add(passed, sink.totals + kSourcePassed);
    if (hist) {
#pragma unroll
        for (uint32_t j = 0; j < kBatches; ++j)
            if (occ[j]) atomicAdd(&lds_occ[j * kGroup + sub], (unsigned long long)occ[j]);
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < n_sources * lds_bins; w += kThreads) {
            const uint32_t s = w / lds_bins, b = w % lds_bins, c = lds_hist[w];
            if (c && b < sink.n_bins) atomicAdd(sink.hist + uint64_t(s) * sink.n_bins + b, (unsigned long long)c);
        }
        if (threadIdx.x < n_sources && lds_occ[threadIdx.x]) atomicAdd(sink.totals + kSourceOccurrences + threadIdx.x, lds_occ[threadIdx.x]);
        if (threadIdx.x <= n_sources && lds_share[threadIdx.x]) atomicAdd(sink.totals + kSourceSharing + threadIdx.x, (unsigned long long)lds_share[threadIdx.x]);
    }
}

}  // namespace

hipError_t launch_source_sink(const void *d_staged, uint64_t m, const SourceView &view, const SourceSink &sink, hipStream_t stream) {
    const bool dump = sink.mode == kSourceSinkAppend || sink.mode == kSourceSinkScatter;
    bool ok = sink.totals && sink.flags && view.rows && view.checkpoints && view.n_sources >= 1 && view.n_sources <= kSourceMax && view.stride >= view.n_sources;
    if (sink.mode == kSourceSinkHist) ok = ok && sink.hist && sink.n_bins >= 2;
    else ok = ok && sink.limits && (sink.mode == kSourceSinkCount || dump);
    if (dump) ok = ok && sink.kmers;
    if (sink.mode == kSourceSinkScatter) ok = ok && sink.bitmap && sink.prefix;
    if (!d_staged || !ok) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_source_sink, dim3(capped_grid(m, kPerBlock, 256u * 8u)), dim3(kThreads), 0, stream, static_cast<const Node *>(d_staged), m,
                       reinterpret_cast<const uint4 *>(view.rows), view.checkpoints, view.total, view.n_sources, view.stride, sink);
    return hipGetLastError();
}

}  // namespace msbwt
