// The source colouring of a merged index (source_index.hip): one byte per row, the input the row came from (what
// msbwt_rle_merge_many's out_source holds), and a rank structure over it -- one checkpoint per kSourceBlockRows rows, the count of
// every source in the rows before the block.  k_range_sources turns FM ranges into per-source counts from these two arrays alone.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace msbwt {

constexpr uint32_t kSourceBlockShift = 10, kSourceBlockRows = 1u << kSourceBlockShift;  // rows per checkpoint
constexpr uint32_t kSourceMax = 32;  // sources at the most (kMergeMaxInputs)
// Ranges of at most this many rows are counted byte by byte, without a checkpoint: with l anywhere in its 16-byte chunk they lie in 256
// bytes, two 16-byte chunks per lane of a kGroup-lane group, and no source's count exceeds the byte the group sums it in.
constexpr uint32_t kSourceNarrow = 240;

// counters per checkpoint: n_sources rounded up to a power of two, so a checkpoint never straddles a 128-byte line it need not
inline uint32_t source_stride(uint32_t n_sources) {
    uint32_t s = 1;
    while (s < n_sources) s <<= 1;
    return s;
}

struct SourceSizes {
    uint64_t nblocks;           // blocks of kSourceBlockRows rows, the last one partial
    uint64_t row_bytes;         // the byte vector, padded to whole 256 bytes (the kernels load aligned 16-byte chunks)
    uint64_t checkpoint_bytes;  // (nblocks + 1) checkpoints of source_stride() u64: checkpoint b = the counts in rows [0, b * kSourceBlockRows), the last one the totals
    uint64_t scratch_bytes;     // of the build alone: the per-block counts, source-major, and the scan's sums
};
SourceSizes source_sizes(uint64_t total, uint32_t n_sources);

struct SourceView {
    const uint8_t *rows = nullptr;
    const uint64_t *checkpoints = nullptr;
    uint64_t total = 0;
    uint32_t n_sources = 0, stride = 0;
};

// rows[0 .. total) in HBM -> checkpoints (source_sizes: checkpoint_bytes), through scratch (scratch_bytes).  A byte >= n_sources sets
// *bad (a device word the caller has zeroed) to 1.  Enqueued on the stream; nothing synchronises.
hipError_t launch_source_build(const uint8_t *rows, uint64_t total, uint32_t n_sources, uint64_t *checkpoints, uint64_t *scratch, uint32_t *bad,
                               hipStream_t stream);

// out[q * n_sources + s] = rows of source s in [l[q * stride], h[q * stride]).  l == h: zeros.  l == h == u64::MAX (a query that held a
// code >= 6): all-ones.  l > h or h > total: all-ones and kFlagInternal in *flags; no address is formed from such a row.
hipError_t launch_range_sources(const SourceView &view, const uint64_t *l, const uint64_t *h, uint32_t stride, uint64_t n, uint64_t *out, uint32_t *flags,
                                hipStream_t stream);

}  // namespace msbwt
