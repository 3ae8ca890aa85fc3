// unitig_source_layout of csrc/graph_layouts.hpp on the host (tests/test_colour_layouts.py builds and runs this), in the manner of
// link_layouts.cpp: for every size below every array starts where its kernels may touch it, no array reaches into the next and the
// last ends inside the block's bytes.  It prints the bytes of every layout it checked; the pytest driver holds
// msbwt_unitig_graph_by_source_plan and msbwt_canonical_unitig_graph_by_source_plan to them.
//
// An array's extent is what unitig_sources.hpp says its kernel touches.  Alignment, as read from unitig_sources.hip and spectrum.cpp:
//    8  the range words: uint64_t -- the plain call's l of every node, written by the edge pass, or the canonical call's pairs {l, h}
//       of a chunk's slots, written by the search with a stride of two words -- read a word at a time by k_unitig_source_sums
//    8  the matrix: U x S uint64_t, zeroed by a memset over exactly 8 U S bytes, then only added to by 64-bit atomics
// Both extents are padded to whole multiples of 256 bytes: the block counts as msbwt_rle_spectrum_scratch_bytes counts an allocation.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "graph_layouts.hpp"

using namespace msbwt;

namespace {

struct Array {
    const char *name;
    uint64_t at, bytes, align;
};

uint64_t checks = 0, failures = 0;

void expect(bool ok, const std::string &where, const char *what, const char *name) {
    ++checks;
    if (ok) return;
    ++failures;
    std::printf("FAIL %s: %s (%s)\n", where.c_str(), what, name);
}

void colours(uint64_t range_words, uint64_t U, uint64_t S, bool staged) {
    const UnitigSourceLayout l = unitig_source_layout(range_words, U, S, staged);
    const std::string where = "unitig sources, R = " + std::to_string(range_words) + ", U = " + std::to_string(U) + ", S = " + std::to_string(S) + (staged ? ", staged" : "");
    std::vector<Array> arrays = {{"ranges", l.ranges, 8 * range_words, 8}};
    if (staged) arrays.push_back({"sums", l.sums, 8 * U * S, 8});
    for (size_t i = 0; i < arrays.size(); ++i) {
        const Array &a = arrays[i];
        expect(a.at % a.align == 0, where, "an array is misaligned", a.name);
        const uint64_t next = i + 1 < arrays.size() ? arrays[i + 1].at : l.bytes;
        expect(a.at + a.bytes <= next, where, "an array reaches into the next, or past the end", a.name);
        expect(next - a.at < a.bytes + 256, where, "an array is padded by 256 bytes or more", a.name);
    }
    expect(l.bytes % 256 == 0 && (l.bytes >= 256 || (range_words == 0 && (!staged || U * S == 0))), where, "an allocation counts with 256 bytes at the least", "bytes");
    expect(l.ranges == 0 && (!staged || l.sums % 256 == 0), where, "the arrays do not start where a block is aligned", "sums");
    std::printf("layout %llu %llu %llu %d %llu\n", (unsigned long long)range_words, (unsigned long long)U, (unsigned long long)S, int(staged), (unsigned long long)l.bytes);
}

}  // namespace

int main() {
    // each side of the 256-byte rounding (32 words), one chunk's pairs (2^21 words), the largest number of nodes a plan accepts
    const uint64_t words[] = {0, 1, 31, 32, 33, 2047, 2048, 2049, (1ull << 21) - 1, 1ull << 21, (1ull << 21) + 1, (1ull << 40) - 1};
    const uint64_t unitigs[] = {0, 1, 7, 8, 9, 31, 32, 33, 1ull << 20, (1ull << 40) - 1};
    for (uint64_t R : words)
        for (uint64_t U : unitigs)
            for (uint64_t S : {uint64_t(1), uint64_t(3), uint64_t(4), uint64_t(5), uint64_t(32)})
                for (bool staged : {false, true}) colours(R, U, S, staged);
    // the range words of either call
    expect(unitig_source_range_words(0, false) == 0 && unitig_source_range_words(5, false) == 5, "range words", "the plain call keeps a word a node", "plain");
    expect(unitig_source_range_words(5, true) == 20 && unitig_source_range_words(kCanonicalUnitigChunkSlots / 2, true) == 2 * kCanonicalUnitigChunkSlots &&
               unitig_source_range_words(kCanonicalUnitigChunkSlots / 2 - 1, true) == 2 * kCanonicalUnitigChunkSlots - 4 &&
               unitig_source_range_words(1ull << 39, true) == 2 * kCanonicalUnitigChunkSlots,
           "range words", "the canonical call keeps a pair a slot of a chunk", "canonical");
    // the chunk the canonical call unpacks its words into: 32 bytes a slot, k <= 31 symbols a word
    const CanonicalUnitigLayout big = canonical_unitig_layout(1ull << 30);
    expect(big.chunk_slots == kCanonicalUnitigChunkSlots && big.hist - big.chunk == 32 * big.chunk_slots, "chunk", "a chunk is not 32 bytes a slot", "chunk");
    std::printf("colour layouts: %llu checks, %llu failures\n", (unsigned long long)checks, (unsigned long long)failures);
    return failures ? 1 : 0;
}
