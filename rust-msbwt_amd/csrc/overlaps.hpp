// Read overlaps (overlaps.hip; msbwt_rle_read_overlaps[_device]): each of n queries searched backwards through the index, and at every
// length j >= min_overlap the interval of reads that BEGIN with the last j symbols of the query: [rank('$', l_j), rank('$', h_j)).
// include/msbwt_hip.h, "read overlaps", defines the search on the BWT string alone; here is what the kernels do:
//   search    one 8-lane group a query, kOverlapSlots queries a group side by side.  A step fetches the line of l_j and the line of
//             h_j -- ONE line when both lie in the same block, none for a bound that is T (its ranks are the symbol counts the call
//             brings) -- and takes from those registers the ranks of the next symbol AND of '$': plane blocks by a second popcount and
//             a second header field in a widened group sum, run blocks by a second accumulator in the decode loop, an OVERFLOW run
//             block from its one extra plane-shaped line.  Step 0 needs no line: R_1 = [C[c], C[c + 1]).  The step loop runs
//             t = 0 .. trips inside the kernel, trips = the largest E of the launch, fixed by the host.  Query symbols are read from
//             the query's end backwards (strand 1: from its start forwards, complemented in registers), an aligned 8-byte word where
//             eight symbols of the query lie in one, single bytes at the ragged ends.
//   pass A    (columns nullptr) writes the per-query outputs and the record counts; pass B (columns given) searches again and writes
//             record k of query i at base + rec_offsets[i] + k: one lane of the group, three plain 8-byte stores.
//   prepare   the largest E = min(L, max_overlap) of a launch's queries into counters[kOverlapMaxE], for a form whose offsets the
//             host does not hold; offsets   out[i] = base + scanned counts[i].
// All pointers are device pointers, every count 64 bits wide.  No address is formed from a bound at or beyond `total`, a query at or
// beyond `n`, a symbol outside [offsets[i], offsets[i + 1]) or a record at or beyond `capacity` or its query's own count: *flags |=
// kFlagInternal instead (kFlagInvalidRange for offsets that decrease: that query has length 0; kFlagInvalidSymbol for a BAD_SYMBOL
// stop).  Every loop runs a count the host fixed.  Integer only, plain C++; plain vector stores, atomicAdd, atomicMax and atomicOr.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>

namespace msbwt {

constexpr uint8_t kOverlapEnd = 1, kOverlapEmpty = 2, kOverlapBadSymbol = 3;
constexpr uint32_t kOverlapSlots = 4;  // queries a group keeps in registers, interleaved: up to eight lines in flight a group

// the words of OverlapCall::counters (256 bytes, zeroed once a call): sums over every pass-A launch since; lines: of both passes
constexpr uint32_t kOverlapSymbols = 0, kOverlapRecords = 1, kOverlapEdges = 2, kOverlapEnds = 3, kOverlapEmpties = 4, kOverlapBads = 5, kOverlapLines = 6,
                   kOverlapMaxE = 7, kOverlapCounterWords = 8;
constexpr uint64_t kOverlapCounterBytes = 256;

constexpr uint64_t kOverlapPiece = 1ull << 20;     // the automatic piece
constexpr uint64_t kOverlapMaxPiece = 1ull << 28;  // the largest one
constexpr uint64_t kOverlapLimit = 1ull << 40;     // n, and the symbols of all queries, stay below

struct OverlapCall {
    const void *blocks;  // the index: IndexView's blocks, overflow, block_format, total
    const void *overflow;
    uint32_t format;
    uint64_t total;
    uint64_t start[7];         // C[0 .. 5] and T: rank(c, T) = start[c + 1] - start[c]
    const uint8_t *symbols;    // symbol j of query i is symbols[offsets[i] - origin + j]
    const uint64_t *offsets;   // n + 1 words
    uint64_t origin;
    uint64_t n;                // the queries of this launch; every per-query array below is indexed 0 .. n
    uint64_t min_overlap, max_overlap;  // max_overlap 0: no limit
    uint32_t strand;
    uint64_t trips;            // >= every query's E = min(L, max_overlap)
    uint64_t *rec_counts;      // pass A: n words, the records of every query (nullptr in pass B)
    uint64_t *matched, *edges; // n words each, may be nullptr
    uint8_t *stops;            // n bytes, may be nullptr
    // pass B: all three columns, or none
    const uint64_t *rec_offsets;  // n + 1 words: the exclusive scan of rec_counts
    uint64_t base, capacity;      // record k of query i goes to base + rec_offsets[i] + k, which is below capacity
    uint64_t *lengths, *first, *counts;
    unsigned long long *counters;
    uint32_t *flags;
};

hipError_t launch_overlaps(const OverlapCall &c, hipStream_t stream);
// counters[kOverlapMaxE] = max(itself, the largest min(L, max_overlap) of the n queries)
hipError_t launch_overlap_prepare(const uint64_t *offsets, uint64_t n, uint64_t max_overlap, unsigned long long *counters, uint32_t *flags, hipStream_t stream);
// out[i] = base + scanned[i], i < words
hipError_t launch_overlap_offsets(const uint64_t *scanned, uint64_t words, uint64_t base, uint64_t *out, hipStream_t stream);

// ---- where the arrays of a call's block lie (msbwt_overlap_plan states the sum; scan_words = scan_scratch_words(P + 1)) ----

inline uint64_t overlap_pad(uint64_t x) { return (x + 255) / 256 * 256; }
inline uint64_t overlap_piece_queries(uint64_t n, uint64_t piece) { return std::min(n, piece ? piece : kOverlapPiece); }

struct OverlapLayout {
    uint64_t counters, counts, scan, in_offsets, symbols, out_offsets, matched, edges, stops, bytes;
};
// at a piece of P queries: the counters, the record counts (P + 1 words) and their scan's scratch; a host form stages a piece's query
// offsets and symbols (piece_symbols: the most symbols a piece holds) and its four per-query outputs, whichever are wanted
inline OverlapLayout overlap_layout(uint64_t P, bool host, uint64_t piece_symbols, uint64_t scan_words) {
    OverlapLayout at{};
    uint64_t cursor = 0;
    const auto put = [&](uint64_t bytes) {
        const uint64_t here = cursor;
        cursor += overlap_pad(bytes);
        return here;
    };
    at.counters = put(kOverlapCounterBytes);
    at.counts = put(8 * (P + 1));
    at.scan = put(8 * scan_words);
    if (host) {
        at.in_offsets = put(8 * (P + 1));
        at.out_offsets = put(8 * (P + 1));
        at.matched = put(8 * P);
        at.edges = put(8 * P);
        at.stops = put(P);
        at.symbols = put(piece_symbols);
    }
    at.bytes = cursor;
    return at;
}
// a host form's staged record columns of a piece that emits `records` records: taken after the piece's pass A, given back after its copy
inline uint64_t overlap_column_bytes(uint64_t records) { return records ? 3 * overlap_pad(8 * records) : 0; }

}  // namespace msbwt
