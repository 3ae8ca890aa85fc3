// Canonical unitigs (canonical_unitigs.hip; msbwt_rle_enumerate_canonical_unitigs[_device]): the strand-merged k-mer graph D compacted
// into its non-branching paths, each class of {q, rc(q)} in exactly one unitig exactly once.  include/msbwt_hip.h defines D; here is
// what the kernels do between the canonical walk (canonical.hpp), which leaves the n classes (canonical word, own, other) in walk
// order, and the compaction of unitigs.hpp, which works over slots whatever they came from:
//   doubling   both member words of every class into one array of N = 2n - palindromes keys, the class count as the payload
//   order      the stable 8-bit radix passes of radix_sort.hpp over the low ceil(2k / 8) bytes of the keys (unitig_calls.cpp calls them): slot
//              order is word order from here on.  WORD -> SLOT is a binary search over the sorted keys, ceil(log2 N) + 1 probes at the
//              most; a word that is no node comes back as N, never as a slot.
//   edges      the four (k+1)-mers q.c of every node are written as packed words chunk by chunk, counted by the library's packed
//              search into cnt[4 slot + c], and folded: cc(q.c) = cnt[q][c] + cnt[rc(q')][3 - q0] (q' = q[1:].c, q0 = q's first
//              symbol; a (k+1)-mer that is its own reverse complement counts once), an edge when cc >= min_edge and q' is a node.
//              So every (k+1)-mer WORD is searched once, a class twice (once from each strand), and no word outside D's out-edges.
//   cuts       after launch_unitig_links: a link into or out of a palindromic node, or along q -> rc(q), is taken back
//   choice     after the ranking: of U and rc(U) the one with the smaller head slot stays; the other's head gets kUnitigSkip
// All pointers are device pointers, all slots 64-bit; no address is formed from a slot at or beyond N: *flags |= kFlagInternal instead.
// Integer only, plain C++; every loop is bounded by a count the host fixed (a binary search: 41 steps).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "unitigs.hpp"

namespace msbwt {

constexpr uint64_t kCanonicalUnitigChunkSlots = 1u << 20;  // nodes whose four (k+1)-mers are searched per batch
constexpr uint64_t kCanonicalUnitigFixedBytes = 256;       // the counters below, padded: zeroed by the caller
enum : uint32_t {                                          // words of the counters
    kCanonicalUnitigSeconds = 0,  // second members written (launch_canonical_unitig_double): N = n + this
    kCanonicalUnitigHairpins,     // edges q -> rc(q) (launch_canonical_unitig_fold)
    kCanonicalUnitigCut,          // links taken back (launch_canonical_unitig_cut)
    kCanonicalUnitigEmitted,      // unitigs that stay, the nodes in them, and the circular ones among them (launch_canonical_unitig_choose)
    kCanonicalUnitigEmittedNodes,
    kCanonicalUnitigEmittedCircular,
    kCanonicalUnitigCounterWords
};

// keys[i] = words[i], vals[i] = own[i] + other[i] for i < n; the reverse complement of every word that is not its own, with the same
// payload, appended from n on in no particular order (counters[kCanonicalUnitigSeconds] counts them).  keys, vals: 2 n words.
hipError_t launch_canonical_unitig_double(const uint64_t *words, const uint64_t *own, const uint64_t *other, uint64_t n, uint32_t k, uint64_t *keys, uint64_t *vals,
                                          unsigned long long *counters, uint32_t *flags, hipStream_t stream);
// out[4 j + c] = the (k+1)-mer keys[first + j].c as a packed word, j < m, c < 4
hipError_t launch_canonical_unitig_edge_words(const uint64_t *keys, uint64_t first, uint64_t m, uint64_t *out, hipStream_t stream);
// the edge bytes (zeroed by the caller) and pred[] (as GraphSink::pred_slot) of D from cnt[4 slot + c] = count_kmer(keys[slot].c)
hipError_t launch_canonical_unitig_fold(const uint64_t *keys, uint64_t N, uint32_t k, uint64_t min_edge, const uint64_t *cnt, uint32_t *edge_words, uint64_t *pred,
                                        unsigned long long *counters, uint32_t *flags, hipStream_t stream);
// after launch_unitig_links: a linked-up node that is a palindrome, or whose predecessor is one or is its reverse complement, becomes
// {i, done} again; its link up and its predecessor's link down are cleared; g.counters' links and unfinished go down by one each
hipError_t launch_canonical_unitig_cut(const UnitigNodes &g, uint32_t k, UnitigState *state, unsigned long long *counters, hipStream_t stream);
// after the ranking and launch_unitig_tails: at every tail t with head h, h' = the head of the slot of rc(word[t]); h > h': kUnitigSkip
// at h, else the unitig is counted as emitted
hipError_t launch_canonical_unitig_choose(const UnitigNodes &g, uint32_t k, const UnitigState *state, unsigned long long *counters, hipStream_t stream);

}  // namespace msbwt
