// Unitig links (unitig_links.hip; msbwt_rle_enumerate_[canonical_]unitig_graph[_device]): the edges of the compacted graph, as a table
// of sides.  include/msbwt_hip.h defines sides and entries; here is what the kernels do behind launch_unitig_emit, over the arrays both
// unitig calls hold then -- the sorted words, the edge and link bytes, state[i] = {head, distance} and heads[h] = {nodes before, number}:
//   degrees   the tail of every emitted unitig u writes popcount(out bits of its edge byte) at offsets[2u] and popcount(in bits of its
//             head's) at offsets[2u + 1] -- 0 there for a unitig that is its own mirror, whose flag byte gets bit 1 --, and 0 goes to
//             offsets[2U].  Without offsets the same kernel only counts: counters[kUnitigLinkEntries] += the entries, which is L.
//   scan      the exclusive scan of the 2U + 1 words in place, tiles of kUnitigTileSlots words: per-tile sums, k_scan_tile_sums over
//             them (workgroup.hpp, as the numbering), and the prefix inside every tile.  offsets[2U] = L then.
//   targets   every tail fills side 2u, every head side 2u + 1: the neighbour's word is the tail's shifted left by a symbol (at k = 32 the
//             first symbol shifts out of the word) or the head's shifted right under the predecessor symbol, WORD -> SLOT is a binary
//             search over the sorted words of `probes` steps, fixed by the host, and the entry follows from the slot's head and, where
//             that unitig is not emitted (canonical: kUnitigSkip), from the head of its mirror's slot.
// All pointers are device pointers, all slots, sides and offsets 64-bit; no address is formed from a slot at or beyond n, a unitig at
// or beyond U, a side beyond 2U or an offset at or beyond L: *flags |= kFlagInternal instead.  Integer only, plain C++.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "unitigs.hpp"

namespace msbwt {

// a word of UnitigNodes::counters behind those of unitigs.hpp (zeroed with them): the entries of all sides of the emitted unitigs
constexpr uint32_t kUnitigLinkEntries = 8;
static_assert(kUnitigLinkEntries >= kUnitigCounterWords && (kUnitigLinkEntries + 1) * 8 <= kUnitigFixedBytes, "inside the padded counters, past the compaction's own");
constexpr uint8_t kUnitigFlagOwnMirror = 2;  // bit 1 of a flag byte: the unitig is its own reverse complement (a palindromic node)

inline uint64_t unitig_link_sides(uint64_t U) { return 2 * U + 1; }  // the words of the offsets

// offsets == nullptr: counters[kUnitigLinkEntries] += the entries (heads is not read: the unitigs need no numbers yet).  Else the
// degrees at offsets[2u], offsets[2u + 1] for u < U, 0 at offsets[2U], and out_flags[u] |= kUnitigFlagOwnMirror (out_flags may be
// nullptr).  canonical: heads carry kUnitigSkip, and a palindromic node is a unitig with one side.
hipError_t launch_unitig_link_degrees(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, bool canonical, uint64_t U, uint64_t *offsets,
                                      uint8_t *out_flags, hipStream_t stream);
// offsets[0 .. 2U] become their exclusive prefix sums.  tiles: unitig_tiles(2U + 1) x kUnitigTileBytes of scratch.
hipError_t launch_unitig_link_scan(uint64_t U, uint64_t *offsets, void *tiles, hipStream_t stream);
// targets[offsets[a] .. offsets[a + 1]) for every side a < 2U; probes: the steps of a binary search over n words, ceil(log2 n) + 1
hipError_t launch_unitig_link_targets(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, bool canonical, uint32_t probes, uint64_t U,
                                      uint64_t L, const uint64_t *offsets, uint64_t *targets, hipStream_t stream);

}  // namespace msbwt
