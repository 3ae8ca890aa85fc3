// Left walks (left_walk.hip; msbwt_rle_walk_rows[_device], msbwt_rle_extract_reads[_device]): from each of n BWT rows the LF walk
// r -> C[S[r]] + rank(S[r], r), emitting S[r], until it stands on a '$' or has taken max_steps steps.  include/msbwt_hip.h, "left
// walks", defines the walk on the BWT string alone; here is what the kernels do:
//   walk      one 8-lane group a walk, kLeftWalkSlots walks a group side by side.  A step is ONE 128-byte line: the group reads the
//             symbol at the row out of the line and ranks that symbol from the same registers (plane blocks: three plane bits and the
//             popcounts of rank_ops.hpp's constrain; run blocks: the run that covers the offset, then the clipped run lengths of
//             rank_runs_group; an OVERFLOW block: one more, dependent line of the side array, plane-shaped).  The step loop runs
//             t = 0 .. max_steps inside the kernel -- max_steps + 1 lines at the most, the last one only to see a '$' -- and ends
//             early for a group whose walks have all stopped.  Symbols are packed eight to a register pair and leave as one 8-byte
//             store where the row's address allows, as single bytes (one a lane) at its ragged ends.  Tallies go through LDS to
//             counters[], four atomics a workgroup.
//   reverse   extraction: a piece's walk-order rows (stride max_len, in scratch) turned into reading order at their ragged places,
//             one wave a read; the piece's offsets (base + the exclusive scan of its lengths) go out beside them.
// All pointers are device pointers, every count 64 bits wide.  No address is formed from a row at or beyond `total`, a walk at or
// beyond `n`, a step at or beyond max_steps or a symbol at or beyond `capacity`: *flags |= kFlagInternal instead (kFlagInvalidRange
// for a caller's row or read id that is out of range).  Every loop runs a count the host fixed.  Integer only, plain C++; plain
// vector stores and atomicAdd.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>

namespace msbwt {

constexpr uint8_t kWalkDollar = 1, kWalkMaxSteps = 2, kWalkBadRow = 3;
constexpr uint32_t kLeftWalkSlots = 4;  // walks a group keeps in registers, interleaved: four lines in flight a group, 32 a wave

// the words of LeftWalkCall::counters (256 bytes, zeroed once a call): sums over every walk launched since
constexpr uint32_t kWalkSteps = 0, kWalkDollars = 1, kWalkMaxed = 2, kWalkBad = 3, kWalkCounterWords = 4;
constexpr uint64_t kWalkCounterBytes = 256;

constexpr uint64_t kWalkPiece = 1ull << 20;     // the automatic piece
constexpr uint64_t kWalkMaxPiece = 1ull << 28;  // the largest one: a launch's grid stays far below 2^31 workgroups
constexpr uint64_t kWalkLimit = 1ull << 40;     // max_steps, and the symbols of all rows, stay below

// what every launch of a call shares
struct LeftWalkCall {
    const void *blocks;    // the index: IndexView's blocks, overflow, block_format, total
    const void *overflow;
    uint32_t format;
    uint64_t total;
    uint64_t dollars;      // C['A']: the rows of the '$' block, which are the read ids
    uint64_t max_steps;
    bool ids;              // the rows are read ids: one at or beyond `dollars` is refused (kFlagInvalidRange, BAD_ROW, 0 steps)
    const uint64_t *rows;  // n words, or nullptr: walk j starts at row first_row + j
    uint64_t first_row;
    uint64_t n;            // the walks of this launch; every array below is indexed by the walk, 0 .. n
    uint8_t *symbols;      // n rows of `stride` bytes; the outputs, each may be nullptr
    uint64_t stride;
    uint64_t *steps;
    uint8_t *stops;
    uint64_t *last, *reads;
    unsigned long long *counters;
    uint32_t *flags;
};

hipError_t launch_left_walk(const LeftWalkCall &c, hipStream_t stream);

// Extraction, after the walk of a piece and the exclusive scan of its n lengths in place (offsets[n] = the piece's symbols): read j's
// walk-order row rows[j * stride ..] reversed to out_symbols[offsets[j] ..] -- out_symbols: where the PIECE's first symbol goes, with
// `room` symbols from there on; nullptr: nothing copied --, and out_offsets[j] = base + offsets[j] for j <= n (out_offsets: the
// piece's n + 1 words; nullptr: not wanted).  No symbol at or beyond `room` is written.
hipError_t launch_left_walk_reverse(const uint8_t *rows, uint64_t stride, const uint64_t *offsets, uint64_t n, uint64_t base, uint8_t *out_symbols, uint64_t room,
                                    uint64_t *out_offsets, uint32_t *flags, hipStream_t stream);

// ---- where the arrays of a call's one block lie (msbwt_walk_plan states the first sum; scan_words = scan_scratch_words(P + 1)) ----

inline uint64_t walk_pad(uint64_t x) { return (x + 255) / 256 * 256; }
inline uint64_t walk_piece_walks(uint64_t n, uint64_t piece) { return std::min(n, piece ? piece : kWalkPiece); }
inline bool walk_too_large(uint64_t n, uint64_t max_steps) { return max_steps >= kWalkLimit || (max_steps && n > (kWalkLimit - 1) / max_steps); }

struct WalkLayout {
    uint64_t counters, rows, symbols, steps, stops, last, reads, bytes;
};
// walk_rows at a piece of P walks: the counters; a host form stages a piece's rows, its four narrow outputs and, wanted, its symbols
inline WalkLayout walk_layout(uint64_t P, uint64_t max_steps, bool symbols, bool host) {
    WalkLayout at{};
    uint64_t cursor = 0;
    const auto put = [&](uint64_t bytes) {
        const uint64_t here = cursor;
        cursor += walk_pad(bytes);
        return here;
    };
    at.counters = put(kWalkCounterBytes);
    if (host) {
        at.rows = put(8 * P);
        at.steps = put(8 * P);
        at.last = put(8 * P);
        at.reads = put(8 * P);
        at.stops = put(P);
        if (symbols) at.symbols = put(P * max_steps);
    }
    at.bytes = cursor;
    return at;
}

struct ExtractLayout {
    uint64_t counters, lengths, scan, rows, ids, offsets, symbols, bytes;
};
// extract_reads at a piece of P reads: the counters, the lengths (P + 1 words) and their scan's scratch, the walk-order rows wanted
// with the symbols; a host form stages a piece's ids (given), its offsets (wanted) and its symbols (wanted: at most P max_len)
inline ExtractLayout extract_layout(uint64_t P, uint64_t max_len, bool ids, bool symbols, bool offsets, bool host, uint64_t scan_words) {
    ExtractLayout at{};
    uint64_t cursor = 0;
    const auto put = [&](uint64_t bytes) {
        const uint64_t here = cursor;
        cursor += walk_pad(bytes);
        return here;
    };
    at.counters = put(kWalkCounterBytes);
    at.lengths = put(8 * (P + 1));
    at.scan = put(8 * scan_words);
    if (symbols) at.rows = put(P * max_len);
    if (host) {
        if (ids) at.ids = put(8 * P);
        if (offsets) at.offsets = put(8 * (P + 1));
        if (symbols) at.symbols = put(P * max_len);
    }
    at.bytes = cursor;
    return at;
}

}  // namespace msbwt
