// The bucket-lookup kernel's pieces that the host shares with the device (lookup_kernel.hip): how a key is found in ONE 128-byte bucket
// line of a complete sparse table (sparse_table.hpp), written over a "word i of the line" accessor so that a host program can run the
// very scan the kernel runs (tests/cpp/lookup_scan_host.cpp) -- and, for HIP translation units, the launcher.
//
// When k equals the depth of a complete table the table's range IS the count: a query is one hashed bucket line and nothing else.  A
// line arrives as eight 16-byte pieces, so the scan comes in two halves:
//   lookup_piece_matches  which of the four words of ONE piece carry the wanted tag;
//   lookup_resolve        the pieces' findings put together (a bit per slot) -> the entry, reading the few further fields -- width, the
//                         tag's high byte, the header -- through the accessor.
// lookup_scan_line runs both over a whole line: the scan as the kernel (its accessor reads the line from LDS) and the host run it.
#pragma once
#include <cstdint>

#include "sparse_table.hpp"

namespace msbwt {

// the complete layout with tags of `tag_bits` bits (24, 32 or 40)
MSBWT_HD constexpr SparseLayout lookup_layout(uint32_t tag_bits) { return tag_bits == 40u ? kLayoutXwide : tag_bits == 32u ? kLayoutWide : kLayoutComplete; }

// Bit j: word 4 `piece` + j of the line is the tag word of a slot and holds the wanted low tag.  (An EMPTY slot -- tag word 0 -- matches a
// key whose tag is 0: lookup_resolve tells it by its width.)
MSBWT_HD uint32_t lookup_piece_matches(const SparseLayout &L, uint32_t piece, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t want_lo) {
    const uint32_t tag_mask = L.width_byte ? ~0u : (1u << kSparseWidthShift) - 1u;
    const uint32_t m = ((w0 & tag_mask) == want_lo ? 1u : 0u) | ((w1 & tag_mask) == want_lo ? 2u : 0u) | ((w2 & tag_mask) == want_lo ? 4u : 0u) |
                       ((w3 & tag_mask) == want_lo ? 8u : 0u);
    const uint32_t slots = (1u << L.slots) - 1u;  // tag[i] is word i
    return m & (slots >> (4u * piece)) & 0xFu;
}

struct LookupFound {
    uint32_t width;   // 0: the key is not in this bucket; 1..254: its count; kSparseEscapeWidth: its range lives in the side array
    uint32_t slot;    // where (width != 0)
    uint32_t header;  // how many entries wanted this bucket: > L.slots says that some were displaced to the next one(s)
};

template <class WordAt>
MSBWT_HD uint32_t lookup_byte(uint32_t b, WordAt &&word_at) { return (word_at(b >> 2) >> ((b & 3u) * 8u)) & 0xFFu; }

// cand: bit i = slot i's tag word matched (the lookup_piece_matches of piece p at bits 4 p ..).  A key sits in at most one slot, so the
// candidate that is an entry (width != 0) and has the tag's high byte (40-bit tags; two keys of a probe window may share their low 32
// bits, never all 40) IS the entry; an empty slot never is.  word_at(i) = word i of the line.
template <class WordAt>
MSBWT_HD LookupFound lookup_resolve(const SparseLayout &L, uint32_t cand, uint32_t want_hi, WordAt &&word_at) {
    LookupFound f{0u, 0u, word_at(L.header_byte / 4u) >> 16};
    while (cand != 0u) {
        const uint32_t i = uint32_t(__builtin_ctz(cand));
        cand &= cand - 1u;
        const uint32_t w = L.width_byte ? lookup_byte(L.width_byte + i, word_at) : word_at(i) >> kSparseWidthShift;
        if (w == 0u) continue;
        if (L.tag_hi_byte != 0u && lookup_byte(L.tag_hi_byte + i, word_at) != want_hi) continue;
        f.width = w;
        f.slot = i;
        break;
    }
    return f;
}

// l of the entry in `slot`: the start of its range -- for an ESCAPE entry the index of its {l, h} pair in the side array
template <class WordAt>
MSBWT_HD uint64_t lookup_entry_l(const SparseLayout &L, uint32_t slot, WordAt &&word_at) {
    return (uint64_t(lookup_byte(L.l_hi_byte + slot, word_at)) << 32) | word_at(L.l_lo_word + slot);
}

// the whole scan of one line
template <class WordAt>
MSBWT_HD LookupFound lookup_scan_line(const SparseLayout &L, uint32_t want_lo, uint32_t want_hi, WordAt &&word_at) {
    uint32_t cand = 0;
    for (uint32_t p = 0; 4u * p < L.slots; ++p)  // the pieces that hold tag words
        cand |= lookup_piece_matches(L, p, word_at(4u * p), word_at(4u * p + 1u), word_at(4u * p + 2u), word_at(4u * p + 3u), want_lo) << (4u * p);
    return lookup_resolve(L, cand, want_hi, word_at);
}

// The count a complete table of `depth` symbols (n = 2 depth key bits) gives the key, the way the kernel walks the buckets: its own, then
// -- while the bucket it did not find the key in had displaced entries -- up to `probe` further ones.  line_word(b, i) = word i of bucket
// line b; side_width(j) = h - l of side entry j.
template <class LineWord, class SideWidth>
MSBWT_HD uint64_t lookup_count(const SparseLayout &L, uint64_t key, uint32_t n, uint32_t nbuckets, uint32_t probe, LineWord &&line_word, SideWidth &&side_width) {
    const uint64_t x = sparse_mix(key, n);
    uint32_t b = sparse_bucket(x, n, nbuckets);
    for (uint32_t dist = 0;; ++dist, ++b) {
        const LookupFound f = lookup_scan_line(L, sparse_tag(x, L), sparse_tag_hi(x, L), [&](uint32_t i) { return line_word(b, i); });
        if (f.width == kSparseEscapeWidth) return side_width(lookup_entry_l(L, f.slot, [&](uint32_t i) { return line_word(b, i); }));
        if (f.width != 0u) return f.width;
        if (!(f.header > L.slots && dist < probe)) return 0;
    }
}

}  // namespace msbwt

#if defined(__HIPCC__) || defined(__HIP__)
#include "kernels.hpp"
#include "search_common.hpp"

namespace msbwt {

// Is this count launch one the lookup kernel serves?  Matrix byte queries whose k is the depth of a complete sparse table with 40-bit
// tags, far larger than the caches (IndexView::stream_lines), over plane blocks; at least a tile of them, counted (no ranges), nothing
// asked for that only the lanes kernel knows (search counters, the completion word of one-wave launches, an inline query), and the
// search kernel left to the library (MSBWT_SEARCH=lanes keeps the lanes kernel: the A/B switch).  lookup_kernel.hip has the measurements.
bool lookup_serves(const IndexView &ix, const QuerySource &src, bool reads);
hipError_t launch_lookup(const IndexView &ix, const QuerySource &src, uint32_t *flags, hipStream_t stream);

}  // namespace msbwt
#endif
