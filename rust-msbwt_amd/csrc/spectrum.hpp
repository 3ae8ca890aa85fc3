// The k-mers an index HOLDS (spectrum.hip): the frontier expansion of the sparse-table builder (frontier.hpp) run to depth k, with a
// sink at the last level instead of a table -- a histogram of the range widths (the abundance spectrum), or the (k-mer, count, l)
// records themselves.  All pointers are device pointers; every call synchronises the stream (chunk by chunk: the host steers).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>

#include "kernels.hpp"

namespace msbwt {

constexpr uint32_t kSpectrumMaxK = 32;           // a k-mer is one 2-bit word
constexpr uint64_t kSpectrumMinFrontier = 64;    // fewest nodes a frontier buffer may be capped to (a node's 16 children must fit four times over)
constexpr uint64_t kSpectrumRankRows = 1024;     // rows per rank checkpoint of the sorted dump's bitmap

// what the last walk did (msbwt_rle_spectrum_info)
struct SpectrumInfo {
    uint64_t k = 0, seed_depth = 0;
    uint64_t chunks = 0;    // chunks of seeds that went through every level
    uint64_t retries = 0;   // chunks taken again at half the size after a frontier overflowed
    uint64_t descents = 0;  // single seeds whose subtree did not fit: expanded one step and re-seeded from their children
    uint64_t nodes[kSpectrumMaxK + 1] = {};  // nodes at depth d that survived the pruning; [k]: the k-mers the sink took
};

// where the walk starts: the non-empty entries of a FLAT direct table of flat_depth < k symbols, or (flat == nullptr) the root
struct SpectrumSeeds {
    const void *flat = nullptr;
    int flat_depth = 0;
};

// ---- sizes (pure) ----
// nodes per frontier buffer: `wanted` (msbwt_rle_set_spectrum_frontier), or automatic -- 2^27 when HBM is plentiful, what an eighth of
// the free bytes holds otherwise, 2^16 at least, and never more than the index can fill (a level's nodes are disjoint non-empty ranges)
uint64_t spectrum_frontier_nodes(uint64_t total, uint64_t free_bytes, uint64_t wanted);
uint64_t spectrum_work_bytes(uint64_t frontier_nodes);  // cursors, the re-seeding stack, two frontiers
uint64_t spectrum_rank_bytes(uint64_t total);           // sorted dump: a bit per row, a checkpoint per kSpectrumRankRows rows, the scan's scratch

// ---- the walks ----
// d_hist[min(count, n_bins - 1)] += 1 for every k-mer (d_hist zeroed by the caller); *distinct, *occurrences: host words
hipError_t spectrum_histogram(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, void *d_work, uint64_t frontier_nodes, uint64_t *d_hist, uint64_t n_bins,
                              uint64_t *distinct, uint64_t *occurrences, SpectrumInfo *info, hipStream_t stream);
// *n = k-mers with min_count <= count (<= max_count unless 0); d_rank != nullptr (spectrum_rank_bytes, for a sorted dump): the bit of
// every such k-mer's l is set and the checkpoints are made.  Nodes narrower than min_count are dropped at every level.
hipError_t spectrum_count(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t min_count, uint64_t max_count, void *d_work, uint64_t frontier_nodes,
                          void *d_rank, uint64_t *n, SpectrumInfo *info, hipStream_t stream);
// the records of the same k-mers: appended in the order the expansion produces them (d_rank == nullptr), or each at the rank of its l
// (d_rank as spectrum_count left it: ascending k-mers).  d_counts and d_l may be nullptr.  Nothing is written at or beyond `capacity`
// (*flags |= kFlagInternal should a record ever want to go there).
hipError_t spectrum_dump(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t min_count, uint64_t max_count, void *d_work, uint64_t frontier_nodes,
                         const void *d_rank, uint64_t *d_kmers, uint64_t *d_counts, uint64_t *d_l, uint64_t capacity, uint32_t *flags, SpectrumInfo *info,
                         hipStream_t stream);

// ---- the rank view of a sorted dump: the scratch of spectrum_rank_bytes as bitmap | checkpoints | scan scratch ----
// The counting walk sets the bit of every emitted k-mer's l; spectrum_rank_close makes the checkpoints; the writing walk places each
// record at spectrum_rank_below(l).  Shared with the by-source dump (source_spectrum.hip), whose emitted k-mers have rows of their own too.
struct SpectrumRank {
    uint32_t *bitmap;
    uint64_t *prefix, *scan;
    uint64_t nblocks;
};
SpectrumRank spectrum_rank_view(const void *d_rank, uint64_t total);
hipError_t spectrum_rank_clear(const SpectrumRank &r, hipStream_t stream);  // no row marked
hipError_t spectrum_rank_close(const SpectrumRank &r, hipStream_t stream);  // prefix[b] = marked rows before block b (enqueued; nothing synchronises)
#ifdef __HIP__
// marked rows below row a: the checkpoint, whole words of the block, the word's low bits
__device__ __forceinline__ uint64_t spectrum_rank_below(const uint32_t *__restrict__ bitmap, const uint64_t *__restrict__ prefix, uint64_t a) {
    constexpr uint64_t kWords = kSpectrumRankRows / 32;
    const uint64_t word = a >> 5, first = (a / kSpectrumRankRows) * kWords;
    uint64_t below = prefix[a / kSpectrumRankRows];
    for (uint64_t j = first; j < word; ++j) below += uint32_t(__popc(bitmap[j]));
    return below + uint32_t(__popc(bitmap[word] & ((1u << (uint32_t(a) & 31u)) - 1u)));
}
#endif

// The walk with the last level STAGED instead of sunk (the canonical calls, canonical.hpp): chunk by chunk, after the synchronisation
// that reads the chunk's cursors, per_chunk(d_kmers, m) gets the m >= 1 k-mers of the chunk that are at least `prune` wide as 24-byte
// records {word, l, h} in a frontier buffer, which the next chunk overwrites: what the hook enqueues on `stream` reads them in time,
// what it returns other than hipSuccess ends the walk.  At most frontier_nodes records a chunk; more is a frontier overflow.
using SpectrumChunkHook = std::function<hipError_t(const void *d_kmers, uint64_t m)>;
hipError_t spectrum_stage(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t prune, void *d_work, uint64_t frontier_nodes, const SpectrumChunkHook &per_chunk,
                          SpectrumInfo *info, hipStream_t stream);

}  // namespace msbwt
