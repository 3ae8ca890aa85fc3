// The k-mer graph (kmer_graph.hip; msbwt_rle_enumerate_kmer_graph[_device], msbwt_rle_kmer_graph_degrees): the sorted dump's records
// with one EDGE BYTE each -- bit j: the (k+1)-mer j.q is an edge (a predecessor of q), bit 4 + j: q.j is one (a successor), A C G T ->
// j = 0..3 -- and the 5 x 5 table of (in, out) degrees folded from those bytes.
// How: the counting walk marks every node's l (spectrum_count with the rank scratch), the staging walk (spectrum_stage) hands each
// chunk's nodes {word, l, h} to launch_graph_edges: one step from q gives its (k+1)-mers e = c.q; each e at least min_edge wide is an
// in-edge of q and an out-edge of its prefix p = e[0..k), whose range holds e's -- so p's record is the last mark at or below e.l.
// Both ends of an edge are nodes (a k-mer occurs at least as often as a (k+1)-mer that holds it, and min_edge >= the node threshold),
// so no bit ever looks for a record that is not there.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "kernels.hpp"
#include "spectrum.hpp"

namespace msbwt {

constexpr uint32_t kGraphDegrees = 5;                                // a node has 0..4 predecessors and 0..4 successors
constexpr uint32_t kGraphTableWords = kGraphDegrees * kGraphDegrees;  // table[5 in + out]
constexpr uint64_t kGraphFixedBytes = 256;                           // the table's 25 counters, padded: zeroed by the caller of launch_graph_degrees

// 32-bit words that hold the edge bytes of n records (four records a word, record r in byte r & 3 of word r >> 2)
inline uint64_t graph_edge_words(uint64_t n) { return (n + 3) / 4; }

struct GraphSink {
    const uint32_t *bitmap;        // spectrum.hpp's rank view as spectrum_count left it: the bit of every node's l ...
    const uint64_t *prefix;        // ... and the checkpoints
    uint32_t *edge_words;          // graph_edge_words(n) words, zeroed by the caller: bits are ORed in
    uint64_t n;                    // records: no slot at or beyond it is touched (*flags |= kFlagInternal should a rank ever say so)
    uint64_t min_edge;             // >= 1: a (k+1)-mer narrower than this is no edge
    uint64_t *kmers, *counts, *l;  // the records, each at the rank of its l (every one optional)
    uint32_t *flags;
    uint64_t *pred_slot;           // optional, n words (unitigs.hpp): per in-edge of a node, the slot of the predecessor, at the node's own slot
};

// the m staged nodes {word, l, h} of a chunk (spectrum_stage) -> their records and the edge bits of their in-edges, at both ends
hipError_t launch_graph_edges(const IndexView &ix, const void *d_staged, uint64_t m, const GraphSink &sink, hipStream_t stream);
// d_table[5 in + out] += the records among edge_words' n bytes with that many predecessor and successor bits
hipError_t launch_graph_degrees(const uint32_t *d_edge_words, uint64_t n, uint64_t *d_table, hipStream_t stream);

}  // namespace msbwt
