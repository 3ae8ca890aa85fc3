// csrc/graph_layouts.hpp on the host (tests/test_graph_layouts.py builds and runs this): for every block and every size below, every
// array starts where its kernels may touch it, no array reaches into the next, the last ends at the block's bytes, the zeroed span
// starts at the first array the kernels want zeroed and holds nothing else, and an overlay stays inside what it lies over.
//
// An array's extent here is what the kernel headers say its kernels touch (unitigs.hpp, canonical_unitigs.hpp, kmer_graph.hpp,
// radix_sort.hpp), with the padding those headers name; the totals against the public header's sums are pinned by the *_abi tests.
//
// Alignment, as read from the kernels:
//   16  UnitigState, alignas(16): unitigs.hip and canonical_unitigs.hip load and store a state as one 16-byte struct (state[i],
//       heads[h]) -- both buffers of the plain call, and the states over cnt in the canonical one, whose second buffer starts N states in
//   16  chunk: k_edge_words (canonical_unitigs.hip) stores two ulonglong2 a node, and its launch refuses a pointer with the low four bits set
//    8  every other 64-bit array -- the words, counts and predecessor slots, cnt[4 slot + c], the sort's keys, payloads, histogram and
//       scan (radix_sort.hip and the scan of run_encode.hip index uint64_t one word at a time), both sets of counters and the degree
//       table (unsigned long long atomics), the offsets, the count sums (atomicAdd) -- and the numbering's tiles: TileSums<2> is two
//       uint64_t with alignof 8, read and written a word at a time (k_unitig_tile_sums, k_scan_tile_sums, k_unitig_number)
//    4  the edge and the link words: uint32_t, four slot bytes a word, ORed atomically (kmer_graph.hip, unitigs.hip, canonical_unitigs.hip)
//    1  symbols, ends and flags of the outputs: uint8_t stores (k_unitig_emit)
// No kernel of the four files reads these arrays with uint4 or wider; the uint4 loads of kmer_graph.hip are of the index's blocks.
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
    bool zeroed = false;  // its kernels want it zeroed before they run
};
struct Overlay {
    const char *name;
    uint64_t at, bytes, align;
    uint64_t over_at, over_bytes;  // the array it must stay inside
};

uint64_t checks = 0, failures = 0;

void expect(bool ok, const std::string &where, const char *what, const char *name) {
    ++checks;
    if (ok) return;
    ++failures;
    std::printf("FAIL %s: %s (%s)\n", where.c_str(), what, name);
}

constexpr uint64_t kNoZeroedSpan = ~0ull;

void check(const std::string &where, std::vector<Array> arrays, uint64_t bytes, uint64_t zero_from, const std::vector<Overlay> &overlays = {}) {
    std::stable_sort(arrays.begin(), arrays.end(), [](const Array &a, const Array &b) { return a.at < b.at; });
    uint64_t first_zeroed = kNoZeroedSpan;
    for (size_t i = 0; i < arrays.size(); ++i) {
        const Array &a = arrays[i];
        expect(a.at % a.align == 0, where, "an array is misaligned", a.name);
        const uint64_t next = i + 1 < arrays.size() ? arrays[i + 1].at : bytes;
        expect(a.at + a.bytes <= next, where, "an array reaches into the next, or past the end", a.name);
        if (a.zeroed) first_zeroed = std::min(first_zeroed, a.at);
        if (zero_from != kNoZeroedSpan) expect(a.zeroed == (a.at >= zero_from) || a.bytes == 0, where, "the zeroed span and the arrays that want zeros differ", a.name);
    }
    expect(!arrays.empty() && arrays.back().at + arrays.back().bytes == bytes, where, "the last array does not end at the block's bytes", "bytes");
    expect(zero_from == first_zeroed, where, "the zeroed span does not start at the first array that wants zeros", "zero_from");
    for (const Overlay &o : overlays) {
        expect(o.at % o.align == 0, where, "an overlay is misaligned", o.name);
        expect(o.at >= o.over_at && o.at + o.bytes <= o.over_at + o.over_bytes, where, "an overlay leaves what it lies over", o.name);
    }
}

void graph_tail(uint64_t n) {
    const GraphTailLayout l = graph_tail_layout(n);
    check("graph tail, n = " + std::to_string(n), {{"table", l.table, kGraphFixedBytes, 8, true}, {"edge_words", l.edge_words, 4 * graph_edge_words(n), 4, true}}, l.bytes, l.zero_from);
}

void unitig_nodes(uint64_t n) {
    const UnitigNodeLayout l = unitig_node_layout(n);
    check("unitig nodes, n = " + std::to_string(n),
          {{"states[0]", l.states[0], 16 * n, 16},
           {"states[1]", l.states[1], 16 * n, 16},
           {"kmers", l.kmers, 8 * n, 8},
           {"counts", l.counts, 8 * n, 8},
           {"pred", l.pred, 8 * n, 8},
           {"tiles", l.tiles, unitig_tiles(n) * kUnitigTileBytes, 8},
           {"counters", l.counters, kUnitigFixedBytes, 8, true},
           {"edge_words", l.edge_words, 4 * graph_edge_words(n), 4, true},
           {"link_words", l.link_words, 4 * graph_edge_words(n), 4, true}},
          l.bytes, l.zero_from);
}

void canonical_unitig_nodes(uint64_t n) {
    const CanonicalUnitigLayout l = canonical_unitig_layout(n);
    const uint64_t M = 2 * n;
    const std::string where = "canonical unitig nodes, n = " + std::to_string(n);
    expect(l.chunk_slots == std::min(M, kCanonicalUnitigChunkSlots), where, "the chunk is not the slots up to the cap", "chunk_slots");
    expect(l.classes[0] + 8 * n <= l.classes[1] && l.classes[1] + 8 * n <= l.classes[2], where, "the walk's columns, alive together, overlap", "classes");
    for (int p = 0; p < 2; ++p) {  // the sort's result in pair p: pred lives beside the keys and payloads that are read from then on
        check(where + ", sorted into pair " + std::to_string(p),
              {{"cnt", l.cnt, 32 * M, 8},
               {"pairs[0].keys", l.pairs[0].keys, 8 * M, 8},
               {"pairs[0].vals", l.pairs[0].vals, 8 * M, 8},
               {"pairs[1].keys", l.pairs[1].keys, 8 * M, 8},
               {"pairs[1].vals", l.pairs[1].vals, 8 * M, 8},
               {"chunk", l.chunk, 32 * l.chunk_slots, 16},
               {"hist", l.hist, 8 * radix_sort_hist_words(M), 8},
               {"scan", l.scan, 8 * radix_sort_scan_words(M), 8},
               {"tiles", l.tiles, unitig_tiles(M) * kUnitigTileBytes, 8},
               {"counters", l.counters, kUnitigFixedBytes, 8, true},
               {"own_counters", l.own_counters, kCanonicalUnitigFixedBytes, 8, true},
               {"edge_words", l.edge_words, 4 * graph_edge_words(M), 4, true},
               {"link_words", l.link_words, 4 * graph_edge_words(M), 4, true}},
              l.bytes, l.zero_from,
              {{"classes[0]", l.classes[0], 8 * n, 8, l.cnt, 32 * M},
               {"classes[1]", l.classes[1], 8 * n, 8, l.cnt, 32 * M},
               {"classes[2]", l.classes[2], 8 * n, 8, l.cnt, 32 * M},
               {"states", l.states, 2 * M * 16, 16, l.cnt, 32 * M},
               {"pred", l.pred[p], 8 * M, 8, l.pairs[1 - p].keys, 8 * M}});
    }
}

void unitig_outputs(uint64_t U, uint64_t S, unsigned staged) {
    const bool sums = staged & 1, symbols = staged & 2, ends = staged & 4, flags = staged & 8;
    const UnitigOutputLayout l = unitig_output_layout(U, S, sums, symbols, ends, flags);
    const auto whole_words = [](uint64_t bytes) { return (bytes + 7) / 8 * 8; };  // a staged byte column is padded to a word: what follows is 64-bit
    std::vector<Array> arrays = {{"offsets", l.offsets, 8 * U + 256, 8}};  // U + 1 words, padded: the last array where nothing is staged
    if (sums) arrays.push_back({"sums", l.sums, 8 * U, 8});
    if (symbols) arrays.push_back({"symbols", l.symbols, whole_words(S), 1});
    if (ends) arrays.push_back({"ends", l.ends, whole_words(U), 1});
    if (flags) arrays.push_back({"flags", l.flags, whole_words(U), 1});
    check("unitig outputs, U = " + std::to_string(U) + ", S = " + std::to_string(S) + ", staged = " + std::to_string(staged), arrays, l.bytes, kNoZeroedSpan);
}

}  // namespace

int main() {
    // each side of every rounding: 4 the edge words, 2048 the numbering's tiles, 4096 the sort's tiles over 2 n slots, 2^19 where 2 n
    // crosses the chunk's cap of 2^20 slots; the last is the largest n a plan accepts
    const uint64_t sizes[] = {0, 1, 3, 4, 5, 2047, 2048, 2049, 4095, 4096, 4097, 1ull << 19, (1ull << 19) + 1, (1ull << 40) - 1};
    for (uint64_t n : sizes) {
        graph_tail(n);
        unitig_nodes(n);
        canonical_unitig_nodes(n);
    }
    for (uint64_t U : {1, 7, 8, 9})
        for (uint64_t S : {1, 7, 8, 9})
            for (unsigned staged = 0; staged < 16; ++staged) unitig_outputs(U, S, staged);
    std::printf("graph layouts: %llu checks, %llu failures\n", (unsigned long long)checks, (unsigned long long)failures);
    return failures ? 1 : 0;
}
