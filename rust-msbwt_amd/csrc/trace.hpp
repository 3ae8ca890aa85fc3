// Traces (trace.hip; msbwt_rle_trace_kmers[_device]): from each of n seed k-mers a walk through the k-mer graph G(k, m, me), node by
// node in one direction under one rule, all walks of a batch advancing together.  include/msbwt_hip.h defines the walk (its steps
// 0-8, the modes, the stop codes); here is what the kernels do BETWEEN two searches -- the searches themselves are the library's
// packed search (launch_count_2bit), a round at a time for all live walks at once:
//   seed      a piece's walks: the seed masked to 2k bits becomes the walk's state, its node query (the seed, searched at length k)
//             goes to queries[j] and the four edges of its fan (searched at k + 1) to queries[walks + 4j ..]
//   round     one thread a live walk, over the counts of that walk's queries.  Round 0 tests the seed (step 0) and looks at its fan;
//             a later round holds a CANDIDATE, chosen a round earlier, with the counts of the candidate's fan and, in unitig mode,
//             of its back-fan: steps 4 and 5 (a merge, the seed again), 6 (the candidate is entered: its symbol goes to the walk's
//             own row, the edge's count to its sum), 7 (the target), then 1-3 for the node just entered (the step limit, the fan
//             empty, the fan branching) and the choice of the next candidate.  A walk that stops writes its five outputs, once;
//             a walk that goes on moves to the front of the OTHER state buffer -- its place from a prefix sum over the workgroup and
//             one atomic a workgroup on counters[kTraceLive] -- and writes its next 4 or 8 queries there, densely.  Outside unitig
//             mode the seed is recognised when it is chosen (nothing has to be searched for step 5), so the walk stops a round early.
//   not nodes every walk of a batch on an empty index: NOT_A_NODE, the masked seed, zeros
// The order among the survivors depends on timing; results do not, since every walk owns its outputs and its state travels with it.
// All pointers are device pointers, every count 64 bits wide.  No address is formed from a live index at or beyond `live`, a place at
// or beyond `live`, a walk outside [first, first + rows) or a step at or beyond max_steps: *flags |= kFlagInternal instead, and the walk
// stops.  Every loop runs a count the host fixed.  Integer only, plain C++.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace msbwt {

constexpr int kTraceRight = 0, kTraceLeft = 1;
constexpr int kTraceUnique = 0, kTraceUnitig = 1, kTraceGreedy = 2;
constexpr uint8_t kTraceDeadEnd = 1, kTraceBranch = 2, kTraceMerge = 3, kTraceReturned = 4, kTraceTarget = 5, kTraceMaxSteps = 6, kTraceNotANode = 7;

// the words of TraceCall::counters (256 bytes, zeroed once a piece; kTraceLive before every round)
constexpr uint32_t kTraceLive = 0, kTraceSteps = 1, kTraceNotNodes = 2, kTraceLongest = 3, kTraceCounterWords = 4;
constexpr uint64_t kTraceCounterBytes = 256;

// a live walk, 64 bytes: it moves as a whole from one state buffer to the other
struct TraceWalk {
    uint64_t seed;        // masked to 2k bits
    uint64_t cur;         // the node the walk is on
    uint64_t cand;        // round 0: the seed; later: the node chosen, not yet entered
    uint64_t cand_count;  // count_kmer of the edge cur -> cand
    uint64_t edge_sum;
    uint64_t steps;
    uint64_t walk;        // its number in the call: the row of its outputs
    uint64_t meta;        // bits 0-1: the symbol of the edge cur -> cand; bits 4-7: the fan bits of cur
};
static_assert(sizeof(TraceWalk) == 64, "the plan's 128 bytes a walk");

inline uint32_t trace_queries_per_walk(int mode) { return mode == kTraceUnitig ? 8u : 4u; }
// the words of a piece's query block (and of its count block): round 0 asks 1 + 4 a walk, a later round 4 or 8
inline uint64_t trace_query_words(uint64_t walks, int mode) { return walks * (mode == kTraceUnitig ? 8u : 5u); }

// what every launch of a call shares
struct TraceCall {
    uint32_t k;
    int mode, direction;
    uint64_t m, me, max_steps;
    uint64_t first, rows;       // seeds, targets and outputs are indexed by walk - first, which is below rows: the whole call's arrays
                                // (first = 0, rows = n: the device form) or a piece's staged ones (the host form)
    const uint64_t *seeds;      // rows words
    const uint64_t *targets;    // as seeds, or nullptr
    uint8_t *symbols;           // the outputs, each may be nullptr
    uint64_t *steps;
    uint8_t *stops;
    uint64_t *edge_sums, *last;
    uint8_t *fans;
    unsigned long long *counters;
    uint32_t *flags;
};

// the walks [first_walk, first_walk + walks) of the call: state[j], queries[j] and queries[walks + 4j .. + 4)
hipError_t launch_trace_seed(const TraceCall &c, uint64_t first_walk, uint64_t walks, TraceWalk *state, uint64_t *queries, hipStream_t stream);
// One round over in[0 .. live).  round0: counts[j] is the seed's, counts[piece_walks + 4j ..] its fan's; else counts[q j ..] are the
// candidate's fan's and, in unitig mode, counts[q j + 4 ..] its back-fan's (q = trace_queries_per_walk).  Survivors: out[p] and
// queries[q p .. q p + q), p < counters[kTraceLive] afterwards.
hipError_t launch_trace_round(const TraceCall &c, bool round0, uint64_t piece_walks, uint64_t live, const TraceWalk *in, const uint64_t *counts, TraceWalk *out,
                              uint64_t *queries, hipStream_t stream);
// an empty index: every walk of the rows stops NOT_A_NODE
hipError_t launch_trace_not_nodes(const TraceCall &c, hipStream_t stream);

}  // namespace msbwt
