// unitig_link_layout of csrc/graph_layouts.hpp on the host (tests/test_link_layouts.py builds and runs this), in the manner of
// graph_layouts.cpp: for every size below every array starts where its kernels may touch it, no array reaches into the next and the
// last ends at the block's bytes.  It prints the bytes of every layout it checked; the pytest driver holds msbwt_unitig_graph_plan and
// msbwt_canonical_unitig_graph_plan to them.
//
// An array's extent is what unitig_links.hpp says its kernels touch.  Alignment, as read from unitig_links.hip:
//    8  the offsets: 2 U + 1 uint64_t, written a word at a time by k_link_degrees and k_link_scan, read so by k_link_targets; the block
//       pads them as the unitig offsets are padded
//    8  the scan's tiles: TileSums<2>, two uint64_t with alignof 8, a word at a time (k_link_tile_sums, k_scan_tile_sums, k_link_scan)
//    8  the targets: uint64_t, one store an entry (k_link_targets)
// Nothing in the block is zeroed by a memset: k_link_degrees writes every word of the offsets, the tile kernels every tile.
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

void links(uint64_t U, uint64_t L, bool staged) {
    const UnitigLinkLayout l = unitig_link_layout(U, L, staged);
    const std::string where = "unitig links, U = " + std::to_string(U) + ", L = " + std::to_string(L) + (staged ? ", staged" : "");
    std::vector<Array> arrays = {{"offsets", l.offsets, 8 * unitig_link_sides(U), 8}, {"tiles", l.tiles, unitig_tiles(unitig_link_sides(U)) * kUnitigTileBytes, 8}};
    if (staged) arrays.push_back({"targets", l.targets, 8 * L, 8});
    std::stable_sort(arrays.begin(), arrays.end(), [](const Array &a, const Array &b) { return a.at < b.at; });
    for (size_t i = 0; i < arrays.size(); ++i) {
        const Array &a = arrays[i];
        expect(a.at % a.align == 0, where, "an array is misaligned", a.name);
        const uint64_t next = i + 1 < arrays.size() ? arrays[i + 1].at : l.bytes;
        expect(a.at + a.bytes <= next, where, "an array reaches into the next, or past the end", a.name);
    }
    expect(arrays.back().at + arrays.back().bytes == l.bytes, where, "the last array does not end at the block's bytes", "bytes");
    expect(l.tiles - l.offsets == 16 * U + 256, where, "the offsets are not padded as the header's plan says", "offsets");
    expect(l.bytes >= 256, where, "an allocation counts with 256 bytes at the least", "bytes");
    std::printf("layout %llu %llu %d %llu\n", (unsigned long long)U, (unsigned long long)L, int(staged), (unsigned long long)l.bytes);
}

}  // namespace

int main() {
    // each side of every rounding: 2048 sides a tile of the scan (U = 1023 has 2047 sides, 1024 has 2049), 1024 tiles a round of
    // k_scan_tile_sums; the last is the largest U a plan accepts
    const uint64_t sizes[] = {0, 1, 2, 1023, 1024, 1025, (1ull << 20) - 1, 1ull << 20, (1ull << 20) + 1, (1ull << 40) - 1};
    for (uint64_t U : sizes)
        for (uint64_t L : {uint64_t(0), uint64_t(1), U, 2 * U + 1, 8 * U})
            for (bool staged : {false, true}) links(U, L, staged);
    std::printf("link layouts: %llu checks, %llu failures\n", (unsigned long long)checks, (unsigned long long)failures);
    return failures ? 1 : 0;
}
