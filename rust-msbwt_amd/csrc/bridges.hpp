// Bridges (bridges.hip; msbwt_rle_bridge_kmers[_device]): for each of n pairs (seed, target) every walk of the k-mer graph G(k, m, me)
// that leads from the seed into the target within a window of lengths, a budget of written rows and a budget of live walks.
// include/msbwt_hip.h defines the exploration (its steps 0-1, the levels W and E, the stop codes); here is what the kernels do BETWEEN
// two searches -- the searches themselves are the library's packed search (launch_count_2bit), a round at a time for the whole frontier:
//   seed      a piece's pairs: pair j's seed and target, masked, go to queries[j] and queries[pairs + j] (searched at length k), the
//             four edges of the seed's fan to queries[2 pairs + 4j ..] (at k + 1); state[j] is the empty walk standing on the seed,
//             and the pair's rows of lengths and edge sums are zeroed
//   start     one thread a pair reads the two node counts: NO_SEED, NO_TARGET, or (max_steps == 0) MAX_STEPS at depth 0 -- or the
//             pair is ALIVE, and counters[kBridgeAlive] counts it
//   a round r = 1, 2, ... over the frontier W(r-1), `live` states in the order (pair, walk order), and the 4 counts a state:
//   decide    one thread a state: the edges of its fan at least me wide are its children; those that enter the target, r >= lo, are
//             bridges, the others go on.  Both masks go into the state's own word, both numbers onto the pair's two counters (one
//             64-bit atomic a wave and counter where the wave holds one pair, else one a lane), and the first state of a pair says
//             where the pair starts
//   verdict   one thread a pair of the piece: found += bridges, then the four stops in the header's precedence; a pair that stops
//             writes found, stop, depth and live and is alive no longer
//   weigh     one thread a state: its scan word -- children in the low half if its pair is still alive, bridges in the high half
//   (scan)    run_encode.hip's exclusive_scan over the `live` words, in place: STABLE, so a child's slot follows from the order of
//             the frontier alone and the next level is in (pair, walk order) again, whatever the timing
//   scatter   one thread a state: each child to its slot of the OTHER buffer -- the parent's row of packed symbols with one more --
//             and its 4 next queries to the same slot; each bridge numbered below max_paths into its row of the outputs.  The last
//             state writes the size of the next level to counters[kBridgeLive], which the host reads once a round.
// One writer per plain store: a state is one thread's in a round, a pair's outputs the verdict's (or start's) of the round that stops
// it, a bridge row the one thread's whose number it carries.
// A state is kBridgeHeadWords + ceil(max_steps / 32) words: FIXED-SIZE ROWS, not a parent-pointer arena -- DESIGN.md 3 "Bridges" says why.
// All pointers are device pointers, every count 64 bits wide.  No address is formed from a state at or beyond `live`, a slot at or
// beyond `slots`, a pair outside the piece or [first, first + rows), or a step at or beyond max_steps: *flags |= kFlagInternal instead,
// and the state is dropped.  Every loop runs a count the host fixed.  Integer only, plain C++.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace msbwt {

constexpr int kBridgeRight = 0, kBridgeLeft = 1;
constexpr uint8_t kBridgeExhausted = 1, kBridgeFull = 2, kBridgeMaxSteps = 3, kBridgeTooWide = 4, kBridgeNoSeed = 5, kBridgeNoTarget = 6;

constexpr uint64_t kBridgeMaxStepsCap = 4096;       // a state stays below 1.1 KB
constexpr uint64_t kBridgeMaxLiveCap = 1ull << 24;  // and a pair's level within a scan word's half
constexpr uint64_t kBridgeSlotsCap = 1ull << 28;
constexpr uint64_t kBridgeSlots = 1ull << 20;       // the automatic frontier of a piece

// the words of BridgeCall::counters (256 bytes, zeroed once a piece)
constexpr uint32_t kBridgeLive = 0, kBridgeAlive = 1, kBridgeExpanded = 2, kBridgeFound = 3, kBridgeCounterWords = 4;
constexpr uint64_t kBridgeCounterBytes = 256;

// a state's words: the head, then its symbols at 2 bits, symbol s in word s / 32 at bit 2 (s % 32)
constexpr uint32_t kBridgePair = 0, kBridgeNode = 1, kBridgeSteps = 2, kBridgeEdgeSum = 3, kBridgeMasks = 4, kBridgeHeadWords = 8;
inline uint64_t bridge_state_words(uint64_t max_steps) { return kBridgeHeadWords + (max_steps + 31) / 32; }

// a pair's words in the piece's table
constexpr uint32_t kPairChildren = 0, kPairBridges = 1, kPairFound = 2, kPairBase = 3, kPairFirst = 4, kPairAlive = 5, kBridgePairWords = 6;

// the pairs of a piece and the states of its frontier: a pair that goes on holds at most max_live states
inline uint64_t bridge_piece_pairs(uint64_t n, uint64_t max_live, uint64_t slots) {
    const uint64_t s = slots ? slots : kBridgeSlots;
    return n < s / max_live ? n : (s / max_live ? s / max_live : 1);
}
inline uint64_t bridge_piece_slots(uint64_t pairs, uint64_t max_live) { return pairs * max_live; }
// the words of a piece's query block (and of its count block): round 0 asks 2 + 4 a pair, a later round 4 a state
inline uint64_t bridge_query_words(uint64_t pairs, uint64_t slots) { return 4 * slots > 6 * pairs ? 4 * slots : 6 * pairs; }

// what every launch of a call shares
struct BridgeCall {
    uint32_t k;
    int direction;
    uint64_t m, me, lo, max_steps, max_paths, max_live;
    uint64_t first, rows;       // inputs and outputs are indexed by pair - first, which is below rows: the whole call's arrays
                                // (first = 0, rows = n: the device form) or a piece's staged ones (the host form)
    const uint64_t *seeds;      // rows words
    const uint64_t *targets;
    uint8_t *symbols;           // the outputs, each may be nullptr: rows x max_paths x max_steps
    uint64_t *lengths;          // rows x max_paths
    uint64_t *edge_sums;
    uint64_t *found;            // rows
    uint8_t *stops;
    uint64_t *depths, *live;
    unsigned long long *counters;
    uint32_t *flags;
};

// A piece: the pairs [first_pair, first_pair + pairs) of the call, their table of kBridgePairWords words a pair, a frontier of `slots`
// states of `words` words in each of two buffers, a scan word a slot.
struct BridgePiece {
    uint64_t first_pair, pairs, slots, words;
    unsigned long long *table;
    uint64_t *weights;
};

hipError_t launch_bridge_seed(const BridgeCall &c, const BridgePiece &p, uint64_t *state, uint64_t *queries, hipStream_t stream);
// counts[j] the seed's, counts[pairs + j] the target's
hipError_t launch_bridge_start(const BridgeCall &c, const BridgePiece &p, const uint64_t *counts, hipStream_t stream);
// Round `round` >= 1 over in[0 .. live), fan_counts[4j ..] the counts of state j's fan: decide, verdict and weigh, the caller's scan
// over p.weights[0 .. live), then scatter -- out[s] and queries[4s ..], s < counters[kBridgeLive] afterwards.
hipError_t launch_bridge_decide(const BridgeCall &c, const BridgePiece &p, uint64_t round, uint64_t live, uint64_t *in, const uint64_t *fan_counts, hipStream_t stream);
hipError_t launch_bridge_scatter(const BridgeCall &c, const BridgePiece &p, uint64_t round, uint64_t live, const uint64_t *in, const uint64_t *fan_counts, uint64_t *out,
                                 uint64_t *queries, hipStream_t stream);
// an empty index: every pair of the rows stops NO_SEED
hipError_t launch_bridge_no_seeds(const BridgeCall &c, hipStream_t stream);

}  // namespace msbwt
