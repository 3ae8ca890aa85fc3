// gfx950 (MI355X, CDNA4): the source colouring of a merged index -- the rank structure over the byte-per-row source vector and the
// second phase of msbwt_rle_count_kmers_by_source, FM ranges -> rows per source.
//
// The rows of input i inside the merged range of a k-mer are exactly the occurrences of the k-mer in input i, so the per-source counts
// of [l, h) are rank_i(h) - rank_i(l) over the source vector: nothing of the index proper is read, and no knob can change a result.
//
// Layout (source_index.hpp): the vector as the merge leaves it, one byte per row, and one checkpoint per kSourceBlockRows rows holding
// every source's count in the rows before the block, 64 bits each, source_stride() counters apart (a power of two: 1..16 sources read
// one 128-byte line per bound, 17..32 two).
//
// Build: k_source_block_counts histograms each block in LDS and raises *bad for a byte >= n_sources; the counts lie source-major,
// one column more than there are blocks, so ONE pass of run_encode.hip's exclusive scan over the whole array gives every source's
// running count (plus what the sources before it hold in all: taken off again by k_source_checkpoints, which also transposes into
// the block-major checkpoints; the last column becomes the totals).
//
// Query: one kGroup-lane group per range, as k_kmer_extensions.  A range of at most kSourceNarrow rows -- a present 31-mer at 30 x
// has some 30 -- is counted from its own bytes: lane j loads chunks j and j + 8 of the 256 bytes from l's 16-byte chunk on, bytes
// outside [l, h) are overwritten with 0xFF, and a loop over the sources compares all four bytes of a dword at once (SWAR equality,
// popcount); four sources' counts travel in the bytes of one dword through one group sum.  No checkpoint is read.  A wider range is
// rank(h) - rank(l): each bound its checkpoint plus the bytes from its block's start, at most 64 chunks, counted the same way.
// Per-source counters never sit in an array indexed at run time (that would live in scratch memory): the loop over sources keeps
// one count at a time and lane s & 7 of the group holds source s until eight of them leave as one 64-byte store.
// The counting itself (source_count.hpp) is shared with the by-source k-mer sink (source_spectrum.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "rank_ops.hpp"
#include "run_encode.hpp"
#include "search_common.hpp"
#include "source_count.hpp"
#include "source_index.hpp"

namespace msbwt {
namespace {

constexpr uint32_t kThreads = 256;
static_assert(kSourceBlockRows == kThreads * 4, "k_source_block_counts: one dword of rows per thread");

// counts[s * columns + b] = rows of source s in block b (columns = nblocks + 1, the last column stays zero)
__global__ __launch_bounds__(256) void k_source_block_counts(const uint32_t *__restrict__ rows4, uint64_t total, uint32_t n_sources, uint64_t nblocks,
                                                             uint64_t *__restrict__ counts, uint32_t *__restrict__ bad) {
    __shared__ uint32_t hist[kSourceMax];
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        if (threadIdx.x < kSourceMax) hist[threadIdx.x] = 0u;
        __syncthreads();
        const uint64_t first = (b << kSourceBlockShift) + threadIdx.x * 4u;
        if (first < total) {
            const uint32_t w = rows4[first >> 2];  // (the vector is padded to whole 256 bytes)
            const uint32_t live = uint32_t(min(uint64_t(4), total - first));
            bool wrong = false;
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t s = (w >> (8u * i)) & 0xFFu;
                if (i < live) {
                    if (s < n_sources) atomicAdd(&hist[s], 1u);
                    else wrong = true;
                }
            }
            if (wrong) atomicOr(bad, 1u);
        }
        __syncthreads();
        if (threadIdx.x < n_sources) counts[uint64_t(threadIdx.x) * (nblocks + 1) + b] = hist[threadIdx.x];
        __syncthreads();
    }
}

// scanned: the exclusive scan of the whole source-major array; checkpoint b of source s = scanned[s][b] - scanned[s][0]
__global__ __launch_bounds__(256) void k_source_checkpoints(const uint64_t *__restrict__ scanned, uint64_t columns, uint32_t n_sources, uint32_t stride,
                                                            uint64_t *__restrict__ checkpoints) {
    const uint64_t words = columns * stride, step = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < words; i += step) {
        const uint64_t b = i / stride;
        const uint32_t s = uint32_t(i % stride);
        checkpoints[i] = s < n_sources ? scanned[uint64_t(s) * columns + b] - scanned[uint64_t(s) * columns] : 0ull;
    }
}

__global__ __launch_bounds__(256) void k_range_sources(const uint4 *__restrict__ rows16, const uint64_t *__restrict__ checkpoints, uint64_t total,
                                                       uint32_t n_sources, uint32_t stride, const uint64_t *__restrict__ ls, const uint64_t *__restrict__ hs,
                                                       uint32_t range_stride, uint64_t n, uint64_t *__restrict__ out, uint32_t *__restrict__ flags) {
    const uint32_t sub = threadIdx.x & (kGroup - 1);
    const uint64_t ngroups = (uint64_t(gridDim.x) * blockDim.x) / kGroup;
    for (uint64_t q = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup; q < n; q += ngroups) {
        const uint64_t l = ls[q * range_stride], h = hs[q * range_stride];
        uint64_t *row = out + q * n_sources;
        if (l == h || h > total || l > h) {  // empty: zeros.  The all-ones range of a query with a code >= 6, or a range no search produces: all-ones
            const uint64_t fill = l == h && h <= total ? 0ull : ~0ull;
            if (fill && !(l == ~0ull && h == ~0ull) && sub == 0u) atomicOr(flags, kFlagInternal);
            for (uint32_t s = sub; s < n_sources; s += kGroup) row[s] = fill;
        } else if (h - l <= kSourceNarrow) {
            const NarrowRows r = narrow_rows(rows16, l, h, sub);
#pragma unroll 1
            for (uint32_t s0 = 0; s0 < n_sources; s0 += 4u) {  // sources s0 .. s0 + 3 in the four bytes of one dword: at most 32 each here, kSourceNarrow summed
                const uint32_t packed = narrow_four(r, s0);
                if (sub < 4u && s0 + sub < n_sources) row[s0 + sub] = (packed >> (8u * sub)) & 0xFFu;
            }
        } else {
            uint64_t mine = 0;  // source s in lane s & 7
#pragma unroll 1
            for (uint32_t s = 0; s < n_sources; ++s) {
                const uint64_t count = wide_count(rows16, checkpoints, stride, l, h, s, sub);
                if (sub == (s & 7u)) mine = count;
                if ((s & 7u) == 7u || s + 1u == n_sources) {
                    if ((s & ~7u) + sub <= s) row[(s & ~7u) + sub] = mine;
                }
            }
        }
    }
}

}  // namespace

SourceSizes source_sizes(uint64_t total, uint32_t n_sources) {
    SourceSizes z;
    z.nblocks = (total + kSourceBlockRows - 1) >> kSourceBlockShift;
    z.row_bytes = (total + 255) / 256 * 256;
    z.checkpoint_bytes = ((z.nblocks + 1) * source_stride(n_sources) * 8 + 255) / 256 * 256;
    const uint64_t words = uint64_t(n_sources) * (z.nblocks + 1);
    z.scratch_bytes = (words + scan_scratch_words(words)) * 8;
    return z;
}

hipError_t launch_source_build(const uint8_t *rows, uint64_t total, uint32_t n_sources, uint64_t *checkpoints, uint64_t *scratch, uint32_t *bad,
                               hipStream_t stream) {
    const SourceSizes z = source_sizes(total, n_sources);
    const uint64_t columns = z.nblocks + 1, words = uint64_t(n_sources) * columns;
    hipError_t e = hipMemsetAsync(scratch, 0, words * 8, stream);
    if (e != hipSuccess) return e;
    if (z.nblocks) {
        hipLaunchKernelGGL(k_source_block_counts, dim3(uint32_t(z.nblocks < 65536 ? z.nblocks : 65536)), dim3(kThreads), 0, stream,
                           reinterpret_cast<const uint32_t *>(rows), total, n_sources, z.nblocks, scratch, bad);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = exclusive_scan(scratch, words, scratch + words, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_source_checkpoints, dim3(grid_for(columns * source_stride(n_sources))), dim3(kThreads), 0, stream, scratch, columns, n_sources,
                       source_stride(n_sources), checkpoints);
    return hipGetLastError();
}

hipError_t launch_range_sources(const SourceView &view, const uint64_t *l, const uint64_t *h, uint32_t stride, uint64_t n, uint64_t *out, uint32_t *flags,
                                hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_range_sources, dim3(grid_for(n * kGroup)), dim3(kThreads), 0, stream, reinterpret_cast<const uint4 *>(view.rows), view.checkpoints,
                       view.total, view.n_sources, view.stride, l, h, stride, n, out, flags);
    return hipGetLastError();
}

}  // namespace msbwt
