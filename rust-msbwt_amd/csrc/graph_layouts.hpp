// Where the arrays of a graph or unitig call lie in its HBM blocks (graph_calls.cpp, unitig_calls.cpp and trace_calls.cpp include this).  One function per
// block returns the byte offset of every array, the block's bytes and -- where the kernels want a tail of it zeroed -- where that tail
// starts: a msbwt_*_plan and the hipMalloc take `bytes`, the call carves `base + field`, the memset runs from `zero_from` to `bytes`.
// A struct lists its arrays in their order in HBM, and its function puts their extents down in that order: the n-th put() is the n-th
// field.  hipMalloc aligns a block to 256 bytes; what precedes a 16-byte array is a multiple of 16, what precedes a 64-bit one of 8
// (tests/cpp/graph_layouts.cpp, link_layouts.cpp for the link table and colour_layouts.cpp for the block by source hold every layout
// to that, and to no array reaching into the next).
#pragma once
#include <algorithm>
#include <cstdint>

#include "bridges.hpp"
#include "canonical_trace.hpp"
#include "canonical_unitigs.hpp"
#include "kmer_graph.hpp"
#include "radix_sort.hpp"
#include "trace.hpp"
#include "unitig_links.hpp"
#include "unitigs.hpp"

namespace msbwt {

static_assert(kGraphTableWords * 8 <= kGraphFixedBytes && kUnitigCounterWords * 8 <= kUnitigFixedBytes && kCanonicalUnitigCounterWords * 8 <= kCanonicalUnitigFixedBytes,
              "the counters fit their padded sizes");
static_assert(sizeof(UnitigState) == 16 && kUnitigTileBytes == 16, "two words a state, and a tile");

struct LayoutCursor {
    uint64_t bytes = 0;  // laid out so far
    uint64_t put(uint64_t extent) { return (bytes += extent) - extent; }
};

// The tail of the graph call's block, behind the records a host dump stages: the degree counters, padded, and the edge words of n records.
struct GraphTailLayout {
    uint64_t table, edge_words, bytes, zero_from = table;
};
inline GraphTailLayout graph_tail_layout(uint64_t n) {
    LayoutCursor c;
    return {c.put(kGraphFixedBytes), c.put(4 * graph_edge_words(n)), c.bytes};
}

// The nodes of the unitig call, n slots: the ranking's two buffers of states, the edge pass's words, counts and predecessor slots, the
// numbering's tiles, the counters, padded, and a byte a slot of edges and of links.
struct UnitigNodeLayout {
    uint64_t states[2], kmers, counts, pred, tiles, counters, edge_words, link_words, bytes, zero_from = counters;
};
inline UnitigNodeLayout unitig_node_layout(uint64_t n) {
    LayoutCursor c;
    return {{c.put(16 * n), c.put(16 * n)}, c.put(8 * n), c.put(8 * n), c.put(8 * n), c.put(unitig_tiles(n) * kUnitigTileBytes), c.put(kUnitigFixedBytes),
            c.put(4 * graph_edge_words(n)), c.put(4 * graph_edge_words(n)), c.bytes};
}

// The nodes of the canonical unitig call: n classes, M = 2 n slots of which the N <= M that doubling fills are used.
//   cnt                 4 M words: cnt[4 slot + c]
//   pairs               the sort's two (keys, payloads), M words an array
//   chunk               the four (k+1)-mer words of chunk_slots nodes at a time
//   hist .. link_words  the sort's histogram and scan, the numbering's tiles, the compaction's counters and this call's own, both
//                       padded, a byte a slot of edges and of links
// and, each inside what it is written over:
//   classes[3]          the walk's records (word, own, other), n words a column, at the start of cnt until doubling has read them
//   states              2 M states over cnt once the fold has read it; the ranking's second buffer starts N states in
//   pred[p]             M words, where the sort left its result in pair p: the keys of the other pair
struct CanonicalUnitigLayout {
    struct Pair {
        uint64_t keys, vals;
    };
    uint64_t cnt;
    Pair pairs[2];
    uint64_t chunk, hist, scan, tiles, counters, own_counters, edge_words, link_words, bytes, zero_from = counters;
    uint64_t chunk_slots = 0, classes[3] = {}, states = cnt, pred[2] = {pairs[1].keys, pairs[0].keys};
};
inline CanonicalUnitigLayout canonical_unitig_layout(uint64_t n) {
    const uint64_t M = 2 * n, chunk_slots = std::min(M, kCanonicalUnitigChunkSlots);
    LayoutCursor c;
    CanonicalUnitigLayout l{c.put(32 * M), {{c.put(8 * M), c.put(8 * M)}, {c.put(8 * M), c.put(8 * M)}}, c.put(32 * chunk_slots), c.put(8 * radix_sort_hist_words(M)),
                            c.put(8 * radix_sort_scan_words(M)), c.put(unitig_tiles(M) * kUnitigTileBytes), c.put(kUnitigFixedBytes), c.put(kCanonicalUnitigFixedBytes),
                            c.put(4 * graph_edge_words(M)), c.put(4 * graph_edge_words(M)), c.bytes};
    l.chunk_slots = chunk_slots;
    for (uint64_t column = 0; column < 3; ++column) l.classes[column] = l.cnt + column * 8 * n;
    return l;
}

// The outputs of either unitig call, U unitigs of S symbols: the offsets (U + 1 words, padded), then whichever of the other four
// columns a host form stages, a byte column padded to whole words -- a column that is not staged takes no room.
struct UnitigOutputLayout {
    uint64_t offsets, sums, symbols, ends, flags, bytes;
};
inline UnitigOutputLayout unitig_output_layout(uint64_t U, uint64_t S, bool sums, bool symbols, bool ends, bool flags) {
    LayoutCursor c;
    return {c.put(8 * U + 256), c.put(sums ? 8 * U : 0), c.put(symbols ? (S + 7) / 8 * 8 : 0), c.put(ends ? (U + 7) / 8 * 8 : 0), c.put(flags ? (U + 7) / 8 * 8 : 0), c.bytes};
}

// The link table of either unitig graph call, U unitigs with L entries: the offsets of the 2 U + 1 sides (padded), the tiles of their
// scan, then the targets where a host form stages them -- a device form's are the caller's own and take no room.
struct UnitigLinkLayout {
    uint64_t offsets, tiles, targets, bytes;
};
inline UnitigLinkLayout unitig_link_layout(uint64_t U, uint64_t L, bool targets) {
    LayoutCursor c;
    return {c.put(16 * U + 256), c.put(unitig_tiles(unitig_link_sides(U)) * kUnitigTileBytes), c.put(targets ? 8 * L : 0), c.bytes};
}

// The block of a unitig graph call by source: the range words -- the plain call's l of every node, or the canonical call's pairs {l, h}
// of a chunk of slots -- then the U x `sources` matrix where a host form stages it; a device form's is the caller's own and takes no
// room.  Both extents are whole multiples of 256 bytes, so a block that holds either is no smaller than what hipMalloc hands out.
struct UnitigSourceLayout {
    uint64_t ranges, sums, bytes;
};
inline UnitigSourceLayout unitig_source_layout(uint64_t range_words, uint64_t U, uint64_t sources, bool sums) {
    const auto padded = [](uint64_t bytes) { return (bytes + 255) / 256 * 256; };
    LayoutCursor c;
    return {c.put(padded(8 * range_words)), c.put(sums ? padded(8 * U * sources) : 0), c.bytes};
}
// the range words of either call: a word a node, or a pair a slot of a chunk of the 2 x `classes` slots
inline uint64_t unitig_source_range_words(uint64_t nodes, bool canonical) { return canonical ? 2 * std::min(2 * nodes, kCanonicalUnitigChunkSlots) : nodes; }

// The one block of a trace call, P walks a piece: the counters, padded, the two state buffers, the queries and their counts -- 1 + 4
// words a walk in round 0, 4 or 8 in a later round -- and, where a host form stages them, a piece's seeds, targets and six outputs.  A
// device form's are the caller's own and take no room.  Every extent is a whole multiple of 256 bytes.
struct TraceLayout {
    uint64_t counters, states[2], queries, counts, seeds, targets, symbols, steps, stops, edge_sums, last, fans, bytes;
};
inline TraceLayout trace_layout_of(uint64_t P, uint64_t max_steps, uint64_t query_words, bool targets, bool host) {
    const auto padded = [](uint64_t bytes) { return (bytes + 255) / 256 * 256; };
    const uint64_t words = padded(8 * query_words), column = host ? padded(8 * P) : 0, bytes = host ? padded(P) : 0;
    LayoutCursor c;
    return {c.put(kTraceCounterBytes), {c.put(padded(sizeof(TraceWalk) * P)), c.put(padded(sizeof(TraceWalk) * P))}, c.put(words), c.put(words), c.put(column),
            c.put(targets ? column : 0), c.put(host ? padded(P * max_steps) : 0), c.put(column), c.put(bytes), c.put(column), c.put(column), c.put(bytes), c.bytes};
}
inline TraceLayout trace_layout(uint64_t P, uint64_t max_steps, int mode, bool targets, bool host) {
    return trace_layout_of(P, max_steps, trace_query_words(P, mode), targets, host);
}
// The one block of a canonical trace call: the same, with the queries of both strands and of the node clause -- 2 + 8 + 1 words a walk in
// round 0, 8 + 1 or 16 + 2 in a later round (canonical_trace.hpp has where each lies).
inline TraceLayout canonical_trace_layout(uint64_t P, uint64_t max_steps, int mode, bool targets, bool host) {
    return trace_layout_of(P, max_steps, canonical_trace_query_words(P, mode), targets, host);
}

// The one block of a bridge call, P pairs a piece with a frontier of S = P max_live slots: the counters, padded, the pairs' table, the
// two buffers of states, a scan word a slot and the scan's sums (scan_words = scan_scratch_words(S)), the queries and their counts --
// 2 + 4 words a pair in round 0, 4 a state in a later round -- and, where a host form stages them, a piece's seeds, targets and seven
// outputs.  A device form's are the caller's own and take no room.  Every extent is a whole multiple of 256 bytes.
struct BridgeLayout {
    uint64_t counters, table, states[2], weights, scan, queries, counts, seeds, targets, symbols, lengths, edge_sums, found, stops, depths, live, bytes;
};
inline BridgeLayout bridge_layout(uint64_t P, uint64_t max_steps, uint64_t max_paths, uint64_t max_live, bool host, uint64_t scan_words) {
    const auto padded = [](uint64_t bytes) { return (bytes + 255) / 256 * 256; };
    const uint64_t S = bridge_piece_slots(P, max_live), state = padded(8 * bridge_state_words(max_steps) * S), words = padded(8 * bridge_query_words(P, S));
    const uint64_t column = host ? padded(8 * P) : 0, rows = host ? padded(8 * P * max_paths) : 0;
    LayoutCursor c;
    return {c.put(kBridgeCounterBytes), c.put(padded(8 * kBridgePairWords * P)), {c.put(state), c.put(state)}, c.put(padded(8 * S)), c.put(padded(8 * scan_words)),
            c.put(words), c.put(words), c.put(column), c.put(column), c.put(host ? padded(P * max_paths * max_steps) : 0), c.put(rows), c.put(rows), c.put(column),
            c.put(host ? padded(P) : 0), c.put(column), c.put(column), c.bytes};
}

}  // namespace msbwt
