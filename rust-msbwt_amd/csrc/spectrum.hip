// gfx950: the k-mers an index holds -- abundance spectrum and k-mer dump (spectrum.hpp) -- by the frontier walk (frontier_walk.hpp: the
// seeds, the steps, the chunks, retries and descents) run to depth k.  A node's key is its k-mer's packed 2-bit word.  This file is the
// SINK, what happens to the children of the last level --
//     histogram   width h - l -> a bin; bins below kLdsBins in an LDS histogram flushed once per workgroup, wider ones by global atomics
//     count/mark  how many k-mers lie in the count window; for a sorted dump the bit of each one's l in a bitmap over the rows
//     append      the records, wherever the workgroup's reservation puts them
//     scatter     the records, each at rank(l) of the bitmap: ranges of distinct k-mers are disjoint and in lexicographic order, so
//                 the number of marked rows below l IS the record's place in ascending k-mer order -- no sort
// -- the rank view of the sorted dump, and the entry points.  The canonical calls (canonical.hip) STAGE instead: the last level is
// materialised by the step that fills every other frontier, and the chunk's k-mers {word, l, h} are handed to the caller's hook before
// the next chunk overwrites them; a last frontier that overflows is a frontier that overflows.
// A count window [m, ..] prunes: a k-mer never occurs more often than any of its suffixes, so a node narrower than m is dropped at
// every level (the spectrum itself does not prune).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "frontier_walk.hpp"
#include "run_encode.hpp"
#include "spectrum.hpp"

namespace msbwt {
namespace {

static_assert(kSpectrumMaxK == kWalkMaxDepth && kSpectrumMinFrontier == kWalkMinFrontier, "the header's constants are the walker's");
// the sink's words of the cursor block
constexpr int kOut = kWalkSink;        // append sink: records written so far
constexpr int kOccur = kWalkSink + 1;  // histogram sink: sum of the widths

constexpr uint32_t kLdsBins = 2048;  // counts below this are tallied in LDS (8 KB): almost all of a read set's mass
constexpr int kSinkHist = 0, kSinkCount = 1, kSinkAppend = 2, kSinkScatter = 3;
constexpr uint32_t kRankWords = uint32_t(kSpectrumRankRows / 32);

__device__ __forceinline__ void block_add64(uint64_t mine, unsigned long long *acc) {  // one atomic per wave
    const unsigned long long s = wave_sum<unsigned long long>(mine);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(acc, s);
}

struct Sink : PlainSink {
    int mode;
    uint64_t min, max;             // the count window (max: all-ones = none)
    unsigned long long *hist;      // kSinkHist
    uint64_t n_bins;
    uint32_t *bitmap;              // kSinkCount (optional), kSinkScatter
    const uint64_t *prefix;        // kSinkScatter: marked rows before every kSpectrumRankRows rows
    uint64_t *kmers, *counts, *l;  // the dumps (counts, l optional)
    uint64_t capacity;
    uint32_t *flags;

    static constexpr uint32_t kLdsWords = kLdsBins;
    struct Thread {
        uint64_t occurrences = 0;
    };
    __device__ __forceinline__ bool keeps(uint64_t width) const { return width >= min && width <= max; }
    __device__ __forceinline__ void begin(uint32_t *lds_hist) const {
        if (mode != kSinkHist) return;
        for (uint32_t b = threadIdx.x; b < kLdsBins; b += kFrontierThreads) lds_hist[b] = 0u;
        __syncthreads();
    }
    __device__ __forceinline__ uint64_t place(uint32_t mine, unsigned long long *cur) const { return mode == kSinkAppend ? reserve(mine, cur + kOut) : 0ull; }
    __device__ __forceinline__ void take(Thread &t, uint32_t *lds_hist, unsigned long long *, uint64_t key, uint64_t a, uint64_t b, uint64_t &at) const {
        const uint64_t width = b - a;
        if (mode == kSinkHist) {
            const uint64_t bin = ::min(width, n_bins - 1u);
            if (bin < kLdsBins) atomicAdd(&lds_hist[bin], 1u);
            else atomicAdd(hist + bin, 1ull);
            t.occurrences += width;
        } else if (mode == kSinkCount) {
            if (bitmap) atomicOr(bitmap + (a >> 5), 1u << (uint32_t(a) & 31u));
        } else {
            uint64_t place = at++;
            if (mode == kSinkScatter) place = spectrum_rank_below(bitmap, prefix, a);
            if (place < capacity) {
                kmers[place] = key;
                if (counts) counts[place] = width;
                if (l) l[place] = a;
            } else {
                atomicOr(flags, kFlagInternal);
            }
        }
    }
    __device__ __forceinline__ void end(Thread &t, uint32_t *lds_hist, unsigned long long *cur) const {
        if (mode != kSinkHist) return;
        __syncthreads();
        const uint32_t bins = uint32_t(::min(uint64_t(kLdsBins), n_bins));
        for (uint32_t b = threadIdx.x; b < bins; b += kFrontierThreads) {
            const uint32_t c = lds_hist[b];
            if (c) atomicAdd(hist + b, (unsigned long long)c);
        }
        block_add64(t.occurrences, cur + kOccur);
    }
};

// the walk with `sink` (hook: staged instead); what it did goes to *info
hipError_t walk_to(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t prune, const Sink &sink, void *d_work, uint64_t frontier_nodes, SpectrumInfo *info,
                   hipStream_t stream, uint64_t *occurrences = nullptr, const SpectrumChunkHook *hook = nullptr) {
    Walker<Sink> walker(ix, seeds.flat, seeds.flat_depth, k, prune, sink, d_work, frontier_nodes, stream, hook);
    const hipError_t e = walker.run();
    const WalkRecord &rec = walker.record();
    *info = SpectrumInfo{};
    info->k = k;
    info->seed_depth = walker.seed_depth();
    info->chunks = rec.chunks;
    info->retries = rec.retries;
    info->descents = rec.descents;
    std::copy(rec.nodes, rec.nodes + kSpectrumMaxK + 1, info->nodes);
    if (occurrences && e == hipSuccess) *occurrences = walker.cursor(kOccur);
    return e;
}

// checkpoint b = marked rows in block b of the bitmap (scanned afterwards)
__global__ __launch_bounds__(256) void k_spectrum_block_marks(const uint32_t *__restrict__ bitmap, uint64_t nblocks, uint64_t *__restrict__ prefix) {
    for (uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; b < nblocks; b += uint64_t(gridDim.x) * blockDim.x) {
        const uint4 *w = reinterpret_cast<const uint4 *>(bitmap + b * kRankWords);
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRankWords / 4u; ++j) {
            const uint4 v = w[j];
            c += uint32_t(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
        }
        prefix[b] = c;
    }
}

uint64_t rank_blocks(uint64_t total) { return total / kSpectrumRankRows + 1; }

}  // namespace

uint64_t spectrum_frontier_nodes(uint64_t total, uint64_t free_bytes, uint64_t wanted) { return walk_frontier_nodes(total, free_bytes, wanted); }

uint64_t spectrum_work_bytes(uint64_t frontier_nodes) { return walk_work_bytes(frontier_nodes); }

SpectrumRank spectrum_rank_view(const void *d_rank, uint64_t total) {
    SpectrumRank r;
    r.nblocks = rank_blocks(total);
    char *base = static_cast<char *>(const_cast<void *>(d_rank));
    r.bitmap = reinterpret_cast<uint32_t *>(base);
    r.prefix = reinterpret_cast<uint64_t *>(base + r.nblocks * (kSpectrumRankRows / 8));
    r.scan = r.prefix + r.nblocks;
    return r;
}

hipError_t spectrum_rank_clear(const SpectrumRank &r, hipStream_t stream) { return hipMemsetAsync(r.bitmap, 0, r.nblocks * (kSpectrumRankRows / 8), stream); }

hipError_t spectrum_rank_close(const SpectrumRank &r, hipStream_t stream) {
    hipLaunchKernelGGL(k_spectrum_block_marks, dim3(uint32_t(std::min<uint64_t>((r.nblocks + 255) / 256, 2048))), dim3(256), 0, stream, r.bitmap, r.nblocks, r.prefix);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : exclusive_scan(r.prefix, r.nblocks, r.scan, stream);
}

uint64_t spectrum_rank_bytes(uint64_t total) {
    const uint64_t nblocks = rank_blocks(total);
    return nblocks * (kSpectrumRankRows / 8) + (nblocks + scan_scratch_words(nblocks)) * sizeof(uint64_t);
}

hipError_t spectrum_histogram(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, void *d_work, uint64_t frontier_nodes, uint64_t *d_hist, uint64_t n_bins,
                              uint64_t *distinct, uint64_t *occurrences, SpectrumInfo *info, hipStream_t stream) {
    if (n_bins < 2 || !d_hist || !d_work) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = kSinkHist;
    sink.min = 1;
    sink.max = ~0ull;
    sink.hist = reinterpret_cast<unsigned long long *>(d_hist);
    sink.n_bins = n_bins;
    const hipError_t e = walk_to(ix, seeds, k, 1, sink, d_work, frontier_nodes, info, stream, occurrences);
    if (e == hipSuccess) *distinct = info->nodes[k];
    return e;
}

hipError_t spectrum_count(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t min_count, uint64_t max_count, void *d_work, uint64_t frontier_nodes,
                          void *d_rank, uint64_t *n, SpectrumInfo *info, hipStream_t stream) {
    if (!d_work) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = kSinkCount;
    sink.min = std::max<uint64_t>(min_count, 1);
    sink.max = max_count ? max_count : ~0ull;
    SpectrumRank r{};
    if (d_rank) {
        r = spectrum_rank_view(d_rank, ix.total);
        const hipError_t e = spectrum_rank_clear(r, stream);
        if (e != hipSuccess) return e;
        sink.bitmap = r.bitmap;
    }
    hipError_t e = walk_to(ix, seeds, k, sink.min, sink, d_work, frontier_nodes, info, stream);
    if (e != hipSuccess) return e;
    *n = info->nodes[k];
    if (d_rank) {
        if ((e = spectrum_rank_close(r, stream)) != hipSuccess) return e;
        e = hipStreamSynchronize(stream);
    }
    return e;
}

hipError_t spectrum_dump(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t min_count, uint64_t max_count, void *d_work, uint64_t frontier_nodes,
                         const void *d_rank, uint64_t *d_kmers, uint64_t *d_counts, uint64_t *d_l, uint64_t capacity, uint32_t *flags, SpectrumInfo *info,
                         hipStream_t stream) {
    if (!d_work || !d_kmers || !flags) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = d_rank ? kSinkScatter : kSinkAppend;
    sink.min = std::max<uint64_t>(min_count, 1);
    sink.max = max_count ? max_count : ~0ull;
    if (d_rank) {
        const SpectrumRank r = spectrum_rank_view(d_rank, ix.total);
        sink.bitmap = r.bitmap;
        sink.prefix = r.prefix;
    }
    sink.kmers = d_kmers;
    sink.counts = d_counts;
    sink.l = d_l;
    sink.capacity = capacity;
    sink.flags = flags;
    return walk_to(ix, seeds, k, sink.min, sink, d_work, frontier_nodes, info, stream);
}

hipError_t spectrum_stage(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t prune, void *d_work, uint64_t frontier_nodes, const SpectrumChunkHook &per_chunk,
                          SpectrumInfo *info, hipStream_t stream) {
    if (!d_work || !per_chunk) return hipErrorInvalidValue;
    return walk_to(ix, seeds, k, prune, Sink{}, d_work, frontier_nodes, info, stream, nullptr, &per_chunk);  // (staged: the sink takes nothing)
}

}  // namespace msbwt
