// Construction (reads_build.hip): a read set in host memory -> the RLE bytes of its multi-string BWT, in HBM.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace msbwt {

// stages the builder times (host clock around a stream synchronisation at every stage border)
enum ReadsBuildStage {
    kStageCopyIn = 0,   // reads and offsets to HBM
    kStageReadOrder,    // sort of the read-start suffixes + the text laid out in that order
    kStageHistogram,    // terminator bitmap + the 4096-bin histogram
    kStageCollect,      // a piece's suffix positions in text order
    kStageSort,         // key gathers + radix passes
    kStageEmit,         // the symbol before every sorted suffix
    kStageEncode,       // symbols -> RLE bytes
    kStageCopyOut,      // RLE bytes to the caller (timed by the caller)
    kReadsBuildStages
};

struct ReadsBuildPlan {
    uint64_t auto_piece;    // suffixes per piece the free HBM allows
    uint64_t device_bytes;  // HBM the build needs with the piece in force
};

// Pure host arithmetic: `piece` 0 = the automatic one.
ReadsBuildPlan plan_reads_build(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t piece);

struct ReadsBuildOutput {
    uint8_t *d_rle = nullptr;  // hipMalloc'ed, the caller frees it (nullptr when rle_bytes == 0)
    uint64_t rle_bytes = 0;
    uint64_t pieces = 0, largest_piece = 0;
    double stage_ms[kReadsBuildStages] = {};
    std::string what;  // on failure: the step that failed
};

// reads / offsets: host memory, checked by the caller (monotone offsets, every byte a code 1..5 or, with `ascii`, not '$';
// n >= 1; offsets[n] - offsets[0] + n < 2^40).  piece_limit >= 1.  `wide` forces 64-bit positions (otherwise they are
// 32-bit while the text is below 2^32 symbols).
hipError_t build_rle_from_reads(const uint8_t *reads, const uint64_t *offsets, uint64_t n, bool ascii, uint64_t piece_limit, bool wide,
                                hipStream_t stream, ReadsBuildOutput *out);

}  // namespace msbwt
