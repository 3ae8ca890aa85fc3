// Canonical traces (canonical_trace.hip; msbwt_rle_trace_canonical_kmers[_device]): the traces of trace.hpp over the strand-merged
// graph D(k, m, me) of the header's "canonical unitigs" section instead of G.  include/msbwt_hip.h defines the walk; the state of a
// walk (TraceWalk), what a call's launches share (TraceCall), the counters and the guards are trace.hpp's.  What differs BETWEEN two
// searches:
//   counts    a word x counts cc(x) = count(x) + count(rc(x)), a palindrome once: every query goes out with its reverse complement,
//             and the round kernel folds the two counts
//   the node clause   an edge needs its far end to be a node, which the edge's own count does not settle at a palindromic far end (k
//             even, m >= 2: `node_clause`).  Of the four far ends of a fan one at most can be a palindrome -- RIGHT: by the complement
//             of the node's second symbol, LEFT: of its last but one -- and that far end is one more query of length k a fan side.  It
//             is written always; it is searched, and its count read, with node_clause only, and used where the word is a palindrome
//   MIRROR    unitig mode stops where the chosen link is one of the two cuts of the canonical unitigs: on words alone, in the round
//             that chose it
// The queries of a piece of W walks, and their counts at the same places (f = 8 or, in unitig mode, 16 words a walk; e = 1 or 2):
//   round 0       [2j], [2j + 1]                the seed and its reverse complement            length k
//                 [2W + 8j + c], [.. + 4 + c]   the fan's edge by c and its reverse complement length k + 1
//                 [10W + j]                     the fan's far end that can be a palindrome     length k
//   later, place p  [f p + c], [f p + 4 + c]    the candidate's fan, as above                  length k + 1
//                 [f p + 8 + c], [f p + 12 + c] unitig mode: its back-fan
//                 [f W + e p], [f W + e p + 1]  the far end of the fan, (unitig mode) of the back-fan   length k
// which is 11 W words, or 18 W in unitig mode: canonical_trace_query_words.  All pointers are device pointers.  No address is formed
// from a live index or a place at or beyond `live`, a walk outside [first, first + rows) or a step at or beyond max_steps (live <= W is
// the host's): *flags |= kFlagInternal instead, and the walk is dropped.  Every loop runs a count the host fixed.  Integer only, plain C++.
#pragma once
#include "trace.hpp"

namespace msbwt {

constexpr uint8_t kCanonicalTraceMirror = 8;

// the (k+1)-mer queries a live walk and later round, and its far ends of length k
inline uint32_t canonical_trace_edge_queries(int mode) { return mode == kTraceUnitig ? 16u : 8u; }
inline uint32_t canonical_trace_node_queries(int mode) { return mode == kTraceUnitig ? 2u : 1u; }
// the words of a piece's query block (and of its count block): round 0 asks 2 + 8 + 1 a walk, a later round 8 + 1 or 16 + 2
inline uint64_t canonical_trace_query_words(uint64_t walks, int mode) { return walks * (mode == kTraceUnitig ? 18u : 11u); }

// the walks [first_walk, first_walk + walks) of the call: state[j] and round 0's queries
hipError_t launch_canonical_trace_seed(const TraceCall &c, uint64_t first_walk, uint64_t walks, TraceWalk *state, uint64_t *queries, hipStream_t stream);
// One round over in[0 .. live), counts laid out as the queries above with W = piece_walks.  Survivors: out[p] and their queries,
// p < counters[kTraceLive] afterwards.  node_clause: the far ends' counts were searched and are read.
hipError_t launch_canonical_trace_round(const TraceCall &c, bool round0, bool node_clause, uint64_t piece_walks, uint64_t live, const TraceWalk *in,
                                        const uint64_t *counts, TraceWalk *out, uint64_t *queries, hipStream_t stream);

}  // namespace msbwt
