// Merge (merge.hip, merge_many.hip): the RLE bytes of two or more multi-string BWTs -> the RLE bytes of the BWT of the union of
// their read sets, by the interleave iteration of Holt & McMillan 2014 (the reference: bwt_util::pairwise_bwt_merge,
// src/bwt_util.rs:21-141).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace msbwt {

constexpr uint32_t kMergeTile = 4096;  // merged rows one workgroup counts and scatters per iteration

// stages the merge times (host clock around a stream synchronisation at every stage border)
enum MergeStage {
    kMergeCopyIn = 0,  // both RLE streams to HBM
    kMergeDecode,      // RLE bytes -> one byte per symbol
    kMergeIterate,     // the interleave iterations
    kMergeEmit,        // the merged symbols, gathered through the final vector
    kMergeEncode,      // symbols -> RLE bytes
    kMergeCopyOut,     // RLE bytes (and the vector) to the caller (timed by the caller)
    kMergeStages
};

// What the host learns from one RLE stream before anything is launched.
enum class MergeInputStatus { kOk, kInvalidSymbol, kTooLarge };
struct MergeInput {
    uint64_t total = 0;        // symbols the stream encodes
    uint64_t long_pieces = 0;  // entries its long sub-runs take in the decoder's list
};
// A run may span any number of bytes and hold zero digits.  kTooLarge: 2^40 symbols or more.
MergeInputStatus scan_merge_input(const uint8_t *rle, size_t n, MergeInput *out);

// Pure host arithmetic: HBM bytes the merge of two BWTs of total0 and total1 symbols needs, whatever their runs are.
// At most 2.5 x (total0 + total1) + 64 MiB.
uint64_t plan_merge(uint64_t total0, uint64_t total1);

// One input: host memory that scan_merge_input accepted (in: what it said).
struct MergeSpan {
    const uint8_t *rle;
    size_t len;
    MergeInput in;
};

struct MergeOutput {
    uint8_t *d_rle = nullptr;    // hipMalloc'ed, the caller frees it
    uint64_t rle_bytes = 0;
    // the final state, hipMalloc'ed, the caller frees it; its first state_bytes bytes describe the merged rows.  merge_rle_pair: bit
    // i & 7 of byte i >> 3 set = merged row i is input 1's.  merge_rle_many: byte i = the input merged row i came from.
    uint8_t *d_state = nullptr;
    uint64_t state_bytes = 0;
    uint64_t iterations = 0;
    double stage_ms[kMergeStages] = {};
    std::string what;  // on failure: the step that failed
};

// spans: two inputs (n == 2), their totals summing to [1, 2^40).
hipError_t merge_rle_pair(const MergeSpan *spans, size_t n, hipStream_t stream, MergeOutput *out);

// The decoder of merge.hip, which merge_many.hip shares: d_rle[0 .. n) in HBM, a stream scan_merge_input accepted (in: what it
// said) -> d_symbols[0 .. in.total), a byte per symbol; d_rle and d_symbols are 16-byte aligned.  The stream is drained when it returns.
struct Arena;
hipError_t decode(Arena &arena, const uint8_t *d_rle, uint64_t n, const MergeInput &in, uint8_t *d_symbols, hipStream_t stream, const char **what);

// ---- any number of inputs in one pass (merge_many.hip) ----

constexpr uint32_t kMergeMaxInputs = 32;

// Pure host arithmetic: HBM bytes the one-pass merge of up to kMergeMaxInputs BWTs of `total` symbols in all needs, whatever
// their number and their runs are.  At least 2 x total, at most 3.25 x total + 64 MiB.
uint64_t plan_merge_many(uint64_t total);

// spans: 1 <= n <= kMergeMaxInputs inputs, their totals summing to [1, 2^40).
hipError_t merge_rle_many(const MergeSpan *spans, size_t n, hipStream_t stream, MergeOutput *out);

}  // namespace msbwt
