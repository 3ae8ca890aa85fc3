// The device sort of the builders (radix_sort.hip): stable least-significant-digit passes of 8 bits over (64-bit key, payload) pairs
// -- per tile of 4096 keys a digit histogram, the exclusive scan of run_encode.hpp over digits x tiles, a scatter.  The builder from
// reads sorts suffix positions by gathered key words with it (reads_build.hip: 32- or 64-bit positions), the canonical unitigs their
// nodes by k-mer word (unitig_calls.cpp: the class count as the payload).  All pointers are device pointers; integer only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace msbwt {

constexpr uint64_t kRadixSortTile = 4096;  // pairs a workgroup ranks and scatters per pass
constexpr uint32_t kRadixDigitBits = 8;

// what a sort of n pairs needs beside the pairs, in 64-bit words
inline uint64_t radix_sort_tiles(uint64_t n) { return (n + kRadixSortTile - 1) / kRadixSortTile; }
inline uint64_t radix_sort_hist_words(uint64_t n) { return 256 * radix_sort_tiles(n); }
inline uint64_t radix_sort_scan_words(uint64_t n) { return (radix_sort_tiles(n) + 3) / 4 + 8; }  // (>= scan_scratch_words of the histogram: checked per call)

// `passes` stable passes over (keys_a, vals_a)[0 .. n), the first by the 8 bits from `shift0`, each by the next 8, every pass from one
// pair of buffers into the other; *in_b: the result is in the b pair (an odd number of passes, n >= 2).  hist: radix_sort_hist_words(n)
// words, scan: radix_sort_scan_words(n) words.  flags (or nullptr): *flags |= kFlagInternal where a pair's place is not below n (the
// pair is skipped then; the scanned histogram counts exactly n).  Payload: uint32_t or uint64_t.
// MSBWT_SORT_GRID=<workgroups> in the environment: (tests) caps the passes' grids, so that a workgroup takes several tiles.
template <class Payload>
hipError_t radix_sort_passes(uint64_t *keys_a, Payload *vals_a, uint64_t *keys_b, Payload *vals_b, uint64_t n, uint32_t shift0, uint32_t passes, uint64_t *hist,
                             uint64_t *scan, uint32_t *flags, hipStream_t stream, bool *in_b);

}  // namespace msbwt
