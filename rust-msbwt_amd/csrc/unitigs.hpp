// Unitigs (unitigs.hip; msbwt_rle_enumerate_unitigs[_device]): the k-mer graph (kmer_graph.hpp) compacted into its non-branching paths.
// The edge pass leaves, per node of the sorted dump, its word, its count, its edge byte and -- GraphSink::pred_slot -- the slot of a
// predecessor, which is THE predecessor where the node has one.  From there on everything is slot arithmetic over n nodes:
//   links     node i is linked up when in(i) = 1 and out(pred[i]) = 1; it then marks pred[i] as linked down.  A self-loop that is a link
//             is a circular unitig of one node and gets no link bits.
//   ranking   pointer jumping over {ancestor, distance}, double-buffered: every node ends with the slot of its path's head and its
//             distance from it.  The host runs the rounds and stops when one leaves nothing unfinished.
//   cycles    what is unfinished then lies on isolated cycles: min-label jumping finds each cycle's smallest slot, the link into it
//             is cut, and the ranking runs again over those nodes.  Every loop is a round count the host fixed.
//   numbering one scan over the slots of (head, nodes of the unitig that starts here): the unitig's number and the nodes before it.
//   emit      every node writes its last symbol, a head the k - 1 before it, a tail the unitig's ends byte and flag.
// All pointers are device pointers, all slots and offsets 64-bit; no address is formed from a slot at or beyond n, a unitig at or
// beyond U or an offset at or beyond S: *flags |= kFlagInternal instead.  Integer only, plain C++.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace msbwt {

constexpr uint64_t kUnitigTileSlots = 2048;   // slots a workgroup numbers at a time: 256 threads, 8 consecutive slots each
constexpr uint64_t kUnitigFixedBytes = 256;   // the counters below, padded: zeroed by the caller
constexpr uint64_t kUnitigDone = 1ull << 63;  // in a state's distance: the ancestor is the head
constexpr uint64_t kDistance = ~kUnitigDone;  // the distance itself
enum : uint32_t {                             // words of the counters
    kUnitigEdges = 0,    // in-edges of all nodes
    kUnitigLinks,        // edges p -> q with out(p) = 1 and in(q) = 1, a cycle's closing link and a self-loop included
    kUnitigCircular,     // circular unitigs: self-loops (launch_unitig_links) and opened cycles (launch_unitig_cycle_cut)
    kUnitigLongest,      // most nodes of one unitig (launch_unitig_tails)
    kUnitigUnfinished,   // nodes a jumping round (or launch_unitig_links) left short of their head: zeroed by the caller before each
    kUnitigCounterWords
};
// bits of a node's link byte (kOnCycle: at the unitig's first node).  kUnitigSkip, at a first node: the unitig is neither numbered nor
// emitted -- set by the canonical call alone (canonical_unitigs.hpp) between the ranking and the numbering; the plain call never sets it.
enum : uint32_t { kUnitigLinkUp = 1, kUnitigLinkDown = 2, kUnitigOnCycle = 4, kUnitigSkip = 8 };

// {ancestor, distance | kUnitigDone} while ranking; {slot 2^r links up, smallest slot of the 2^r nodes from here up} while a cycle
// looks for its opening; in the other buffer, after the ranking, at a head's slot {nodes of all unitigs before, unitig number}
struct alignas(16) UnitigState {  // (read and written as one 16-byte access)
    unsigned long long x, y;
};

struct UnitigNodes {
    uint64_t n;                  // nodes = slots
    const uint64_t *kmers;       // per slot, as the edge pass left them: the 2-bit word,
    const uint64_t *counts;      // its count,
    const uint64_t *pred;        // the slot of a predecessor (read only where in = 1)
    const uint32_t *edge_words;  // and the edge bytes, four a word
    uint32_t *link_words;        // the link bytes, four a word, zeroed by the caller
    unsigned long long *counters;
    uint32_t *flags;
};

inline uint64_t unitig_tiles(uint64_t n) { return (n + kUnitigTileSlots - 1) / kUnitigTileSlots; }
constexpr uint64_t kUnitigTileBytes = 16;  // per tile: the scan's two sums

// link bytes, state[i] = {i, done} or {pred[i], 1}, and the counters of edges, links, self-loops and unfinished (= linked up) nodes
hipError_t launch_unitig_links(const UnitigNodes &g, UnitigState *state, hipStream_t stream);
// one round: dst[i] = src[i] jumped over src[its ancestor]; counters[kUnitigUnfinished] += the nodes still short of their head
hipError_t launch_unitig_jump(const UnitigNodes &g, const UnitigState *src, UnitigState *dst, hipStream_t stream);
// the unfinished nodes of state become {pred[i], i}
hipError_t launch_unitig_cycle_seed(const UnitigNodes &g, UnitigState *state, hipStream_t stream);
// one round of the min-label jumping over the unfinished nodes (the finished ones are copied)
hipError_t launch_unitig_cycle_jump(const UnitigNodes &g, const UnitigState *src, UnitigState *dst, hipStream_t stream);
// an unfinished node whose label is its own slot opens its cycle: {i, done}, its link up and its predecessor's link down cut, on-cycle
// set, counters[kUnitigCircular] += 1; the others become {pred[i], 1} again and count as unfinished
hipError_t launch_unitig_cycle_cut(const UnitigNodes &g, UnitigState *state, hipStream_t stream);
// every tail writes its unitig's nodes to heads[its head].x; counters[kUnitigLongest] = the most
hipError_t launch_unitig_tails(const UnitigNodes &g, const UnitigState *state, UnitigState *heads, hipStream_t stream);
// heads[h] = {nodes before, number} at every head h, in slot order; offsets[u] = nodes before + u (k - 1) for u < U, offsets[U] = S.
// tiles: unitig_tiles(n) x kUnitigTileBytes of scratch.
hipError_t launch_unitig_number(const UnitigNodes &g, UnitigState *heads, void *tiles, uint32_t k, uint64_t U, uint64_t S, uint64_t *offsets, hipStream_t stream);
// the outputs (each may be nullptr; count_sums zeroed by the caller: the counts are added).  skip_marked: heads carry kUnitigSkip
hipError_t launch_unitig_emit(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, uint64_t U, uint64_t S, uint8_t *symbols,
                              uint64_t *count_sums, uint8_t *ends, uint8_t *out_flags, hipStream_t stream, bool skip_marked = false);

}  // namespace msbwt
