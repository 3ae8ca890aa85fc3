// Unitigs by source (unitig_sources.hip; msbwt_rle_enumerate_[canonical_]unitig_graph_by_source[_device]): per emitted unitig and per
// input of a merged index, the rows of that input in the ranges of the unitig's nodes.  include/msbwt_hip.h defines the column; here
// is what the kernel does behind launch_unitig_emit, over the arrays both unitig calls hold then -- the sorted words, the link bytes,
// state[i] = {head, distance} and heads[h] = {nodes before, number} -- and the source vector with its checkpoints (source_index.hpp):
//   range     of slot first + j, j < m: [l[i], l[i] + counts[i]) where the edge pass kept every node's range start (the plain call), or
//             the pair {pairs[2 j], pairs[2 j + 1]} of a chunk of slots whose words were searched again (the canonical call, whose
//             counts are class counts).  An empty range adds nothing: a member of a class that does not occur.
//   unitig    the number at the head of the slot's unitig; where that head carries kUnitigSkip (canonical), the number at the head of
//             the slot of the reverse complement of the slot's word, found by a binary search of `probes` steps, fixed by the host --
//             so both members of a class add to the one emitted unitig that holds the class, and a palindromic node adds once.
//   counts    by a kGroup-lane group per slot, as the by-source sink counts (source_count.hpp), and sums[u * S + s] += c_s by 64-bit
//             integer atomics, which commute: the matrix is the same from run to run.  sums is zeroed by the caller.
// All pointers are device pointers, all slots and rows 64-bit; no address is formed from a slot at or beyond n, a unitig at or beyond
// U or a row at or beyond the total: *flags |= kFlagInternal instead.  Integer only, plain C++.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "source_index.hpp"
#include "unitigs.hpp"

namespace msbwt {

// the ranges of the slots [first, first + m): l (n words, indexed by slot) or pairs (2 m words, indexed from `first`), the other nullptr
struct UnitigSourceRanges {
    const uint64_t *l, *pairs;
    uint64_t first, m;
};

// sums[u * view.n_sources + s] += the rows of source s in the range of every slot of `ranges` whose unitig u is emitted.
// canonical: heads carry kUnitigSkip; probes: the steps of a binary search over n words, ceil(log2 n) + 1.
hipError_t launch_unitig_source_sums(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, bool canonical, uint32_t probes, uint64_t U,
                                     const SourceView &view, const UnitigSourceRanges &ranges, uint64_t *sums, hipStream_t stream);

}  // namespace msbwt
