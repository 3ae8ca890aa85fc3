// K-mers by source (source_spectrum.hip; msbwt_rle_kmer_spectrum_by_source, msbwt_rle_enumerate_kmers_by_source[_device]): the k-mers
// of a merged index with c_s, their count in every input s -- the rows of source s in the k-mer's range (source_index.hpp) -- as one
// abundance spectrum per input, or as the records (word, c_0 .. c_{S-1}, l) of the k-mers whose counts pass a per-source window.
// How: the walk of spectrum.hip stages a chunk's k-mers {word, l, h} (spectrum_stage) and launch_source_sink counts, judges and emits
// them in ONE kernel: a k-mer's S counts live in the registers of its kGroup-lane group and nowhere else -- no scratch of the sink
// grows with the frontier, let alone with frontier x sources.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "source_index.hpp"

namespace msbwt {

constexpr int kSourceSinkHist = 0, kSourceSinkCount = 1, kSourceSinkAppend = 2, kSourceSinkScatter = 3;
// words of SourceSink::totals
constexpr int kSourcePassed = 0;                                 // k-mers that passed the predicate (count / mark)
constexpr int kSourceOut = 1;                                    // records appended
constexpr int kSourceOccurrences = 8;                            // [8 + s]: the sum of c_s (histogram)
constexpr int kSourceSharing = kSourceOccurrences + kSourceMax;  // [40 + j]: k-mers held by exactly j sources (histogram)
constexpr int kSourceTotalWords = kSourceSharing + kSourceMax + 1;
// The histogram's LDS part: kSourceLdsWords counters shared out evenly, kSourceLdsWords / source_stride(S) low bins per source (4096
// for one source, 128 for 17..32) -- 16 KB at every S; counts beyond them go to the global histogram by atomics.
constexpr uint32_t kSourceLdsWords = 4096;
// fixed device words of a call beside the walk's scratch: the limits (kSourceMax minima, then kSourceMax maxima) and the totals
constexpr uint64_t kSourceSinkFixedBytes = (2 * kSourceMax + kSourceTotalWords + 7) / 8 * 64;

struct SourceSink {
    int mode;
    const uint64_t *limits;          // min_counts[kSourceMax], then max_counts[kSourceMax] (all-ones = none); not read by the histogram
    uint64_t min_total, max_total;   // the window of the sum (max: all-ones = none)
    unsigned long long *hist;        // kSourceSinkHist: hist[s * n_bins + min(c_s, n_bins - 1)] += 1 for c_s >= 1 (bin 0 is the caller's: k-mers - the others)
    uint64_t n_bins;
    uint32_t *bitmap;                // kSourceSinkCount (optional: the bit of every passing k-mer's l), kSourceSinkScatter
    const uint64_t *prefix;          // kSourceSinkScatter: spectrum.hpp's rank checkpoints
    uint64_t *kmers, *counts, *l;    // the dumps: counts n x S row-major; counts and l optional.  Nothing is written at or beyond capacity (*flags |= kFlagInternal)
    uint64_t capacity;
    uint32_t *flags;
    unsigned long long *totals;      // kSourceTotalWords words, zeroed by the caller
};

// the m staged k-mers {word, l, h} of a chunk (spectrum_stage) -> the sink
hipError_t launch_source_sink(const void *d_staged, uint64_t m, const SourceView &view, const SourceSink &sink, hipStream_t stream);

}  // namespace msbwt
