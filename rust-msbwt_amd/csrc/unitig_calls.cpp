// The unitig calls of a loaded index, twelve entry points: the unitigs the k-mer graph compacts into (unitigs.hpp: the graph's walks
// into scratch, then kernels over its slots) or the canonical ones (canonical_unitigs.hpp: the same compaction over both members of
// every canonical class); with the five columns alone, with the link table of the compacted graph behind them (unitig_links.hpp), or
// with the matrix of per-input sums behind that (unitig_sources.hpp); each in a host and a device form.  A caller's arrays come in as
// one UnitigOutputs, whose three parts each keep their allocation, their kernels and their copies; the two bodies differ in how they
// come by the ranked slots.  The frame of a call is walk_call.hpp's, where the arrays of its blocks lie is graph_layouts.hpp's.
#include <optional>

#include "walk_call.hpp"

#include "canonical.hpp"
#include "canonical_unitigs.hpp"
#include "graph_layouts.hpp"
#include "order.hpp"
#include "radix_sort.hpp"
#include "unitig_links.hpp"
#include "unitig_sources.hpp"
#include "unitigs.hpp"

namespace {

// the walks of either call; its nodes (unitig_node_layout, canonical_unitig_layout) and outputs (unitig_output_layout) come on top
constexpr Shape kUnitigShape{true, false, 0, 0};
constexpr Shape kCanonicalUnitigShape{false, true, kCanonicalTotalWords * 8 < 256 ? 256 : kCanonicalTotalWords * 8, 0};  // (fixed: the walk's totals)
static_assert(MSBWT_UNITIG_INFO_WORDS == 8 && MSBWT_CANONICAL_UNITIG_INFO_WORDS == 10, "the header's constants");

// The six plans, each part's block on top of the part before: the walks and the nodes or classes of either call and, unless it is the
// counting call (unitigs = symbols = links = 0), the outputs with all four columns staged (kPlanColumns); behind them the link table
// with its targets staged (kPlanLinks); behind that the block by source with the matrix of `n_sources` columns staged
// (kPlanSources).  What no call can return is refused before a layout sees it.
enum UnitigPlanParts { kPlanColumns, kPlanLinks, kPlanSources };
int unitigs_plan(bool canonical, UnitigPlanParts parts, uint64_t total_rows, uint64_t free_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links,
                 size_t n_sources, uint64_t *device_bytes) {
    if (parts == kPlanSources && (n_sources < 1 || n_sources > kSourceMax)) return MSBWT_ERR_INVALID_ARG;
    if (nodes >= kMaxSymbols || unitigs >= kMaxSymbols || symbols / 33 >= kMaxSymbols || links / 8 >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;  // (S <= 32 n + n, L <= 8 U)
    uint64_t more = canonical ? canonical_unitig_layout(nodes).bytes : unitig_node_layout(nodes).bytes;
    if (unitigs || symbols || links) {
        more += unitig_output_layout(unitigs, symbols, true, true, true, true).bytes;
        if (parts >= kPlanLinks) more += unitig_link_layout(unitigs, links, true).bytes;
        if (parts >= kPlanSources) more += unitig_source_layout(unitig_source_range_words(nodes, canonical), unitigs, n_sources, true).bytes;
    }
    return plan(canonical ? kCanonicalUnitigShape : kUnitigShape, total_rows, free_bytes, nodes, more, device_bytes);
}

// Links, ranking, cycles and tails over the slots of g (unitigs.hpp): every node of `cur` ends with its head and its distance,
// heads[h].x in `other` with the nodes of the unitig that starts at h, c[] with the counters and *rounds with the jumping rounds run.
// after_links() runs between the links and the first look at the counters (the canonical call takes links back there).
template <class AfterLinks>
int rank_unitigs(Frame &f, const UnitigNodes &g, UnitigState *&cur, UnitigState *&other, uint64_t (&c)[kUnitigCounterWords], uint64_t *rounds, AfterLinks &&after_links) {
    msbwt_rle *h = f.h;
    const auto read = [&] { return read_counters(f, g.counters, c); };
    // Ranking rounds until none is unfinished, `cap` at the most.  A round that finishes nobody ends them too: on every path
    // the unfinished node nearest the head has a finished ancestor, so what is left then lies on cycles.
    const auto rank = [&](uint64_t cap) -> int {
        for (uint64_t round = 0; c[kUnitigUnfinished] && round < cap; ++round) {
            const uint64_t before = c[kUnitigUnfinished];
            HIP_TRY(h, hipMemsetAsync(g.counters + kUnitigUnfinished, 0, 8, f.stream));
            HIP_TRY(h, launch_unitig_jump(g, cur, other, f.stream));
            std::swap(cur, other);
            ++*rounds;
            if (int rc = read()) return rc;
            if (c[kUnitigUnfinished] == before) break;
        }
        return MSBWT_OK;
    };
    HIP_TRY(h, launch_unitig_links(g, cur, f.stream));
    if (int rc = after_links()) return rc;
    if (int rc = read()) return rc;
    if (int rc = rank(ceil_log2(g.n) + 1)) return rc;
    if (const uint64_t on_cycles = c[kUnitigUnfinished]) {
        // a cycle has at most on_cycles nodes: after ceil(log2) rounds every label is its cycle's smallest slot
        HIP_TRY(h, launch_unitig_cycle_seed(g, cur, f.stream));
        for (uint64_t round = 0; round < ceil_log2(on_cycles); ++round, ++*rounds) {
            HIP_TRY(h, launch_unitig_cycle_jump(g, cur, other, f.stream));
            std::swap(cur, other);
        }
        HIP_TRY(h, hipMemsetAsync(g.counters + kUnitigUnfinished, 0, 8, f.stream));
        HIP_TRY(h, launch_unitig_cycle_cut(g, cur, f.stream));
        if (int rc = read()) return rc;
        if (int rc = rank(ceil_log2(on_cycles) + 1)) return rc;
    }
    HIP_TRY(h, launch_unitig_tails(g, cur, other, f.stream));
    return read();
}

// What a body hands the outputs once its ranking is done, and what the two calls differ in behind that point.
struct UnitigRanked {
    const UnitigNodes &g;
    const UnitigState *state;  // every node with its head and its distance
    UnitigState *heads;        // heads[h].x: the nodes of the unitig that starts at h
    void *tiles;               // of the numbering's scan
    uint64_t U, S;
    bool canonical;            // heads carry kUnitigSkip, the sides follow the canonical rule, the ranges of the nodes come by search
    uint64_t expect_links;     // what the graph's counters say L is, where they say it (the plain call); ~0: they do not
    uint64_t *chunk;           // canonical: 32 bytes a slot of a chunk (the call's own, free behind the fold) ...
    uint64_t chunk_slots;      // ... and the slots of a chunk
    uint32_t probes() const { return uint32_t(ceil_log2(g.n) + 1); }  // the steps of a binary search over the slots
};

// The link table of a unitig graph call (unitig_links.hpp; the entry point fills the first four members): count() finds L before the
// call looks at its capacities -- so that a capacity below L also writes nothing --, take() is unitig_link_layout in a block of its
// own, run() the degrees, their scan and the targets, behind the emission, whose flag bytes the degrees add to.
struct UnitigLinkTable {
    void *offsets, *targets;  // the caller's: 2 U + 1 words and L words, each may be nullptr
    uint64_t capacity;
    uint64_t *out_links;  // may be nullptr
    uint64_t L = 0;
    Column cols[2] = {};  // the offsets -- the scan needs them, wanted or not --, the targets
    char *tiles = nullptr;

    int count(Frame &f, const UnitigRanked &r) {  // the tails' degrees added up
        uint64_t c[kUnitigLinkEntries + 1] = {};
        HIP_TRY(f.h, launch_unitig_link_degrees(r.g, r.state, nullptr, uint32_t(f.k), r.canonical, r.U, nullptr, nullptr, f.stream));
        if (int rc = read_counters(f, r.g.counters, c)) return rc;
        L = c[kUnitigLinkEntries];
        if (L > 8 * r.U || (r.expect_links != ~0ull && L != r.expect_links))
            return fail(f.h, MSBWT_ERR_INTERNAL, f.name + ": the sides hold " + std::to_string(L) + " entries, which the graph's counters do not bear out");
        if (out_links) *out_links = L;
        return MSBWT_OK;
    }
    int take(Frame &f, uint64_t U) {
        const UnitigLinkLayout at = unitig_link_layout(U, L, f.host && targets);
        char *block = nullptr;
        if (int rc = f.take_more(&block, at.bytes, "for the links")) return rc;
        cols[0] = {offsets, 8, unitig_link_sides(U), at.offsets, true};
        cols[1] = {targets, 8, L, at.targets};
        place(f, cols, block);
        tiles = block + at.tiles;
        return MSBWT_OK;
    }
    int run(Frame &f, const UnitigRanked &r, uint8_t *d_flags) {
        uint64_t *d_offsets = cols[0].as<uint64_t>(), *d_targets = cols[1].as<uint64_t>();
        HIP_TRY(f.h, launch_unitig_link_degrees(r.g, r.state, r.heads, uint32_t(f.k), r.canonical, r.U, d_offsets, d_flags, f.stream));
        HIP_TRY(f.h, launch_unitig_link_scan(r.U, d_offsets, tiles, f.stream));
        if (d_targets) HIP_TRY(f.h, launch_unitig_link_targets(r.g, r.state, r.heads, uint32_t(f.k), r.canonical, r.probes(), r.U, L, d_offsets, d_targets, f.stream));
        return MSBWT_OK;
    }
};

// The U x S matrix of a unitig graph call by source (unitig_sources.hpp; the entry point fills the first member), where the call
// fills buffers and the matrix is wanted.  Its block is unitig_source_layout: the plain call takes the range words before its edge
// walk (take_ranges), which leaves every node's l there, and the rest in take(), behind the link block; run() zeroes the matrix and
// adds the sums up behind the links, the canonical call a chunk of slots at a time behind a search for their ranges.
struct UnitigSourceMatrix {
    void *sums;  // the caller's: U x S words, may be nullptr
    uint64_t *l = nullptr;      // plain: every node's range start, n words
    uint64_t *pairs = nullptr;  // canonical: {l, h} of a chunk of slots
    Column cols[1] = {};

    int take_ranges(Frame &f, uint64_t n) {
        char *block = nullptr;
        if (int rc = f.take_more(&block, unitig_source_layout(unitig_source_range_words(n, false), 0, 0, false).bytes, "for the ranges of the nodes")) return rc;
        l = in<uint64_t>(block, 0);
        return MSBWT_OK;
    }
    int take(Frame &f, const UnitigRanked &r) {
        const uint64_t sources = f.h->sources.n_sources;
        const UnitigSourceLayout at = unitig_source_layout(r.canonical ? 2 * r.chunk_slots : 0, r.U, sources, f.host);
        char *block = nullptr;
        if (at.bytes)
            if (int rc = f.take_more(&block, at.bytes, "for the sums by source")) return rc;
        if (r.canonical) pairs = in<uint64_t>(block, at.ranges);
        cols[0] = {sums, 8 * sources, r.U, at.sums};
        place(f, cols, block);
        return MSBWT_OK;
    }
    int run(Frame &f, const UnitigRanked &r) {
        msbwt_rle *h = f.h;
        const SourceView view = h->sources.view(h->totals.total);
        uint64_t *d_sums = cols[0].as<uint64_t>();
        HIP_TRY(h, hipMemsetAsync(d_sums, 0, cols[0].rows * cols[0].bytes, f.stream));
        if (!r.canonical) {
            HIP_TRY(h, launch_unitig_source_sums(r.g, r.state, r.heads, uint32_t(f.k), false, r.probes(), r.U, view, UnitigSourceRanges{l, nullptr, 0, r.g.n}, d_sums, f.stream));
            return MSBWT_OK;
        }
        // the slots hold words and class counts: a chunk's words as symbol bytes, their ranges by the library's search, the sums
        uint8_t *rows = reinterpret_cast<uint8_t *>(r.chunk);
        for (uint64_t first = 0; first < r.g.n; first += r.chunk_slots) {
            const uint64_t m = std::min(r.chunk_slots, r.g.n - first);
            HIP_TRY(h, launch_unpack_rows(r.g.kmers + first, uint32_t(f.k), m, rows, f.stream));
            if (int rc = timed_with_tickets(h, f.stream, [&](const IndexView &v) {
                    return launch_kmer_ranges(v, rows, uint32_t(f.k), m, pairs, pairs + 1, 2u, h->d_flags + f.which, f.stream);
                }))
                return rc;
            HIP_TRY(h, launch_unitig_source_sums(r.g, r.state, r.heads, uint32_t(f.k), true, r.probes(), r.U, view, UnitigSourceRanges{nullptr, pairs, first, m}, d_sums, f.stream));
        }
        return MSBWT_OK;
    }
};

// The outputs of a unitig call, plain or canonical, as its entry point hands them over: the five columns and the two totals, and with
// them or not the link table and the matrix by source.  open(): the frame's guard ladder with the call's own checks (args) and the
// thresholds' in it, then zeros in the totals and the handle's info words.  emit(), once the slots are ranked, is the sequence it
// reads as; each part allocates before any runs (the blocks: unitig_output_layout, the links', the matrix's).  close(): what a graph
// call that filled nothing still owes.  deliver(): the copies.
struct UnitigOutputs {
    void *symbols, *offsets, *sums, *ends, *flags;  // the caller's: S bytes, U + 1 words, U words, U bytes, U bytes; each may be nullptr
    uint64_t capacity_unitigs, capacity_symbols;
    uint64_t *out_unitigs, *out_symbol_total;  // the second may be nullptr
    std::optional<UnitigLinkTable> links = std::nullopt;
    std::optional<UnitigSourceMatrix> by_source = std::nullopt;
    uint64_t U = 0, S = 0;
    bool filled = false;
    Column cols[5] = {};  // in the block's order: the offsets -- the numbering needs them, wanted or not --, sums, symbols, ends, flags

    // the name the texts say: which call it is follows from the parts that are there
    const char *call(bool canonical) const {
        if (canonical) return by_source ? "enumerate_canonical_unitig_graph_by_source" : links ? "enumerate_canonical_unitig_graph" : "enumerate_canonical_unitigs";
        return by_source ? "enumerate_unitig_graph_by_source" : links ? "enumerate_unitig_graph" : "enumerate_unitigs";
    }
    bool fills() const { return capacity_unitigs || capacity_symbols || (links && links->capacity); }  // (else: the counting call)
    bool colours() const { return by_source && by_source->sums && fills(); }                            // the matrix is wanted, and the call fills buffers

    template <size_t W, class Args>
    int open(Frame &f, const GraphCut &cut, uint64_t (msbwt_rle::*info)[W], Args &&args) const {
        const auto checks = [&] { const int rc = args(); return rc ? rc : cut.check(f, out_unitigs); };
        if (int rc = f.open(by_source.has_value(), checks)) return rc;
        *out_unitigs = 0;
        if (out_symbol_total) *out_symbol_total = 0;
        if (links && links->out_links) *links->out_links = 0;
        std::fill(f.h->*info, f.h->*info + W, 0ull);
        return MSBWT_OK;
    }

    // the plain call's range words, before its edge walk: nullptr where the matrix is not wanted
    int take_ranges(Frame &f, uint64_t n, uint64_t **l) {
        *l = nullptr;
        if (!colours()) return MSBWT_OK;
        if (int rc = by_source->take_ranges(f, n)) return rc;
        *l = by_source->l;
        return MSBWT_OK;
    }

    int emit(Frame &f, const UnitigRanked &r) {
        msbwt_rle *h = f.h;
        U = r.U;
        S = r.S;
        *out_unitigs = U;
        if (out_symbol_total) *out_symbol_total = S;
        if (links)  // L, before anything is written
            if (int rc = links->count(f, r)) return rc;
        if (!fills()) return MSBWT_OK;
        // the capacity contract: every wanted array holds what the call found, or nothing is written
        if (capacity_unitigs < U || (symbols && capacity_symbols < S) || (links && links->targets && links->capacity < links->L)) {
            std::string have = std::to_string(capacity_unitigs) + (links ? ", " : " and ") + std::to_string(capacity_symbols);
            std::string need = "U = " + std::to_string(U) + " unitigs of S = " + std::to_string(S) + " symbols";
            if (links) {
                have += " and " + std::to_string(links->capacity);
                need += " with L = " + std::to_string(links->L) + " links";
            }
            return f.refuse(": the capacities " + have + " are less than the " + need);
        }
        // the blocks
        const auto staged = [&](const void *wanted) { return f.host && wanted; };
        const UnitigOutputLayout at = unitig_output_layout(U, S, staged(sums), staged(symbols), staged(ends), staged(flags));
        char *block = nullptr;
        if (int rc = f.take_more(&block, at.bytes, "for the unitigs")) return rc;
        cols[0] = {offsets, 8, U + 1, at.offsets, true};
        cols[1] = {sums, 8, U, at.sums};
        cols[2] = {symbols, 1, S, at.symbols};
        cols[3] = {ends, 1, U, at.ends};
        cols[4] = {flags, 1, U, at.flags};
        place(f, cols, block);
        if (links)
            if (int rc = links->take(f, U)) return rc;
        if (colours())
            if (int rc = by_source->take(f, r)) return rc;
        // the columns: numbering and emission
        uint64_t *d_sums = cols[1].as<uint64_t>();
        uint8_t *d_flags = cols[4].as<uint8_t>();
        if (d_sums) HIP_TRY(h, hipMemsetAsync(d_sums, 0, 8 * U, f.stream));
        HIP_TRY(h, launch_unitig_number(r.g, r.heads, r.tiles, uint32_t(f.k), U, S, cols[0].as<uint64_t>(), f.stream));
        HIP_TRY(h, launch_unitig_emit(r.g, r.state, r.heads, uint32_t(f.k), U, S, cols[2].as<uint8_t>(), d_sums, cols[3].as<uint8_t>(), d_flags, f.stream, r.canonical));
        // the links, then the sums by source
        if (links)
            if (int rc = links->run(f, r, d_flags)) return rc;
        if (colours())
            if (int rc = by_source->run(f, r)) return rc;
        filled = true;
        return MSBWT_OK;
    }

    // a graph call that had capacities and found nothing to fill (an empty index, no node that counts): side 0 of no unitig starts at 0
    int close(Frame &f, int rc) const {
        if (rc || filled || !links || !links->offsets || !fills()) return rc;
        if (f.host) {
            *static_cast<uint64_t *>(links->offsets) = 0;
            return MSBWT_OK;
        }
        HIP_TRY(f.h, hipMemsetAsync(links->offsets, 0, 8, f.stream));
        HIP_TRY(f.h, hipStreamSynchronize(f.stream));
        return MSBWT_OK;
    }

    int deliver(Frame &f) {
        if (filled) {
            if (int rc = copy_columns(f, cols)) return rc;
            if (links)
                if (int rc = copy_columns(f, links->cols)) return rc;
            if (by_source)
                if (int rc = copy_columns(f, by_source->cols)) return rc;
        }
        if (f.host) return status_of(f.h, f.stream, f.which);  // synchronises
        HIP_TRY(f.h, hipStreamSynchronize(f.stream));           // (the scratch is freed on return)
        return MSBWT_OK;
    }
};

// Both forms: the sorted dump's counting walk, the staged walk with the edge pass behind it (into scratch: words, counts, edge bytes
// and predecessor slots), then links, ranking, cycles, numbering and emission over the slots (unitigs.hpp).
int unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, bool host, hipStream_t stream, UnitigOutputs out) {
    Frame f(bwt, out.call(false), k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = out.open(f, cut, &msbwt_rle::unitig_info, [] { return int(MSBWT_OK); })) return rc;
    msbwt_rle *h = f.h;
    const int rc = two_pass(
        f, ~0ull, nullptr, "k-mers", false, [&](uint64_t *n) { return count_nodes(f, kUnitigShape, cut, n); },
        [&](uint64_t n) -> int {
            const UnitigNodeLayout at = unitig_node_layout(n);
            char *block = nullptr;
            if (int rc = f.take_more(&block, at.bytes, "for the nodes of the graph")) return rc;
            UnitigState *cur = in<UnitigState>(block, at.states[0]), *other = in<UnitigState>(block, at.states[1]);
            uint64_t *kmers = in<uint64_t>(block, at.kmers), *counts = in<uint64_t>(block, at.counts), *pred = in<uint64_t>(block, at.pred);
            uint32_t *edge_words = in<uint32_t>(block, at.edge_words);
            HIP_TRY(h, hipMemsetAsync(block + at.zero_from, 0, at.bytes - at.zero_from, f.stream));
            HIP_TRY(h, hipMemsetAsync(pred, 0xFF, n * 8, f.stream));  // (no slot)
            uint64_t *l = nullptr;
            if (int rc = out.take_ranges(f, n, &l)) return rc;
            if (int rc = graph_edge_walk(f, cut, n, edge_words, kmers, counts, l, pred)) return rc;

            const UnitigNodes g{n, kmers, counts, pred, edge_words, in<uint32_t>(block, at.link_words), in<unsigned long long>(block, at.counters), h->d_flags + f.which};
            uint64_t c[kUnitigCounterWords] = {}, rounds = 0;
            if (int rc = rank_unitigs(f, g, cur, other, c, &rounds, [] { return int(MSBWT_OK); })) return rc;
            if (c[kUnitigUnfinished] || c[kUnitigLinks] > n + c[kUnitigCircular] || c[kUnitigCircular] > n)
                return fail(h, MSBWT_ERR_INTERNAL, f.name + ": the ranking left " + std::to_string(c[kUnitigUnfinished]) + " nodes without a head");
            const uint64_t U = n - c[kUnitigLinks] + c[kUnitigCircular], S = n + U * (k - 1);
            const uint64_t info[MSBWT_UNITIG_INFO_WORDS] = {n, c[kUnitigEdges], c[kUnitigLinks], U, S, c[kUnitigCircular], c[kUnitigLongest], rounds};
            std::copy(info, info + MSBWT_UNITIG_INFO_WORDS, h->unitig_info);
            const uint64_t entries = 2 * (c[kUnitigEdges] - c[kUnitigLinks] + c[kUnitigCircular]);  // (every edge that is no link, and a closing link, from both its ends)
            return out.emit(f, UnitigRanked{g, cur, other, block + at.tiles, U, S, false, entries, nullptr, 0});
        },
        [&](uint64_t) { return out.deliver(f); });
    return out.close(f, rc);
}

// ---- canonical unitigs ----

// Both forms: the canonical walk counts the classes and then appends them; both members of every class become nodes in word order;
// the (k+1)-mers out of every node are counted and folded into D's edge bytes; then the compaction of the plain call over the N
// slots, with the cuts behind the links and the choice between a unitig and its mirror behind the ranking (canonical_unitigs.hpp).
int canonical_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, bool host, hipStream_t stream, UnitigOutputs out) {
    Frame f(bwt, out.call(true), k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = out.open(f, cut, &msbwt_rle::canonical_unitig_info,
                          [&] { return k > 31 ? f.refuse(" needs 1 <= k <= 31 (an edge is a packed (k+1)-mer)") : int(MSBWT_OK); }))
        return rc;
    msbwt_rle *h = f.h;
    CanonicalSink classes{};
    classes.mode = kCanonicalCount;
    classes.min = cut.m;
    classes.max = ~0ull;
    const uint64_t prune = cut.m / 2 + cut.m % 2;  // (enumerate_canonical: the member that emits a class has at least half of its count)
    uint64_t totals[kCanonicalTotalWords] = {};
    const int rc = two_pass(
        f, ~0ull, nullptr, "classes", true,
        [&](uint64_t *n) -> int {
            if (int rc = take_scratch(f, kCanonicalUnitigShape)) return rc;
            if (int rc = canonical_walk(f, prune, classes, totals)) return rc;
            *n = totals[kCanonicalClasses];
            return MSBWT_OK;
        },
        [&](uint64_t n) -> int {
            const CanonicalUnitigLayout at = canonical_unitig_layout(n);  // over M = 2 n slots, with what lies over what
            char *block = nullptr;
            if (int rc = f.take_more(&block, at.bytes, "for the nodes of the graph")) return rc;
            uint64_t *cnt = in<uint64_t>(block, at.cnt), *chunk = in<uint64_t>(block, at.chunk);
            unsigned long long *own_counters = in<unsigned long long>(block, at.own_counters);
            uint32_t *edge_words = in<uint32_t>(block, at.edge_words), *flags = h->d_flags + f.which;
            HIP_TRY(h, hipMemsetAsync(block + at.zero_from, 0, at.bytes - at.zero_from, f.stream));

            // the classes, in walk order
            classes.mode = kCanonicalAppend;
            classes.kmers = in<uint64_t>(block, at.classes[0]);
            classes.own = in<uint64_t>(block, at.classes[1]);
            classes.other = in<uint64_t>(block, at.classes[2]);
            classes.capacity = n;
            classes.flags = flags;
            if (int rc = canonical_walk(f, prune, classes, totals)) return rc;
            if (totals[kCanonicalOut] != n) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": the second walk found another number of classes");

            // the nodes, in word order
            uint64_t own[kCanonicalUnitigCounterWords] = {};
            uint64_t *const sort_keys[2] = {in<uint64_t>(block, at.pairs[0].keys), in<uint64_t>(block, at.pairs[1].keys)};
            uint64_t *const sort_vals[2] = {in<uint64_t>(block, at.pairs[0].vals), in<uint64_t>(block, at.pairs[1].vals)};
            HIP_TRY(h, launch_canonical_unitig_double(classes.kmers, classes.own, classes.other, n, uint32_t(k), sort_keys[0], sort_vals[0], own_counters, flags, f.stream));
            if (int rc = read_counters(f, own_counters, own)) return rc;
            if (own[kCanonicalUnitigSeconds] > n) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": more second members than classes");
            const uint64_t N = n + own[kCanonicalUnitigSeconds];
            bool in_b = false;
            const uint32_t passes = (2 * uint32_t(k) + kRadixDigitBits - 1) / kRadixDigitBits;  // the bytes above 2k bits are zero in every key
            HIP_TRY(h, radix_sort_passes(sort_keys[0], sort_vals[0], sort_keys[1], sort_vals[1], N, 0, passes, in<uint64_t>(block, at.hist), in<uint64_t>(block, at.scan), flags,
                                         f.stream, &in_b));
            const uint64_t *keys = sort_keys[in_b], *vals = sort_vals[in_b];
            uint64_t *pred = in<uint64_t>(block, at.pred[in_b]);  // (in the pair the sort left free)
            HIP_TRY(h, hipMemsetAsync(pred, 0xFF, N * 8, f.stream));  // (no slot)

            // the edges: count_kmer of the four (k+1)-mers out of every node, a chunk of nodes at a time, then the fold
            for (uint64_t first = 0; first < N; first += at.chunk_slots) {
                const uint64_t nodes = std::min(at.chunk_slots, N - first);
                HIP_TRY(h, launch_canonical_unitig_edge_words(keys, first, nodes, chunk, f.stream));
                if (int rc = launch_count_2bit(h, chunk, k + 1, size_t(4 * nodes), cnt + 4 * first, f.stream, f.which)) return rc;
            }
            HIP_TRY(h, launch_canonical_unitig_fold(keys, N, uint32_t(k), cut.me, cnt, edge_words, pred, own_counters, flags, f.stream));

            // the compaction over the N slots (the counts are folded: their place is the states')
            UnitigState *cur = in<UnitigState>(block, at.states), *other = cur + N;
            const UnitigNodes g{N, keys, vals, pred, edge_words, in<uint32_t>(block, at.link_words), in<unsigned long long>(block, at.counters), flags};
            uint64_t c[kUnitigCounterWords] = {}, rounds = 0;
            if (int rc = rank_unitigs(f, g, cur, other, c, &rounds, [&]() -> int {
                    HIP_TRY(h, launch_canonical_unitig_cut(g, uint32_t(k), cur, own_counters, f.stream));
                    return MSBWT_OK;
                }))
                return rc;
            HIP_TRY(h, launch_canonical_unitig_choose(g, uint32_t(k), cur, own_counters, f.stream));
            if (int rc = read_counters(f, own_counters, own)) return rc;
            const uint64_t U = own[kCanonicalUnitigEmitted], circular = own[kCanonicalUnitigEmittedCircular];
            if (c[kUnitigUnfinished] || own[kCanonicalUnitigEmittedNodes] != n || U > n || circular > U)
                return fail(h, MSBWT_ERR_INTERNAL, f.name + ": the ranking left " + std::to_string(c[kUnitigUnfinished]) + " nodes without a head, and the emitted unitigs hold " +
                                                       std::to_string(own[kCanonicalUnitigEmittedNodes]) + " of " + std::to_string(n) + " classes");
            const uint64_t S = n + U * (k - 1);
            const uint64_t info[MSBWT_CANONICAL_UNITIG_INFO_WORDS] = {n, (c[kUnitigEdges] + own[kCanonicalUnitigHairpins]) / 2, n + circular - U, U, S, circular, c[kUnitigLongest], rounds,
                                                              2 * n - N, own[kCanonicalUnitigCut]};
            std::copy(info, info + MSBWT_CANONICAL_UNITIG_INFO_WORDS, h->canonical_unitig_info);
            return out.emit(f, UnitigRanked{g, cur, other, block + at.tiles, U, S, true, ~0ull, chunk, at.chunk_slots});
        },
        [&](uint64_t) { return out.deliver(f); });
    return out.close(f, rc);
}

}  // namespace

extern "C" {

// ---- unitigs: the non-branching paths of the k-mer graph as ragged sequences ----

int msbwt_rle_enumerate_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets, uint64_t *out_count_sums,
                                uint8_t *out_ends, uint8_t *out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs,
                                uint64_t *out_symbol_total) {
    return unitigs(bwt, k, min_count, min_edge, true, nullptr,
                   {out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total});
}

int msbwt_rle_enumerate_unitigs_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                       void *d_out_count_sums, void *d_out_ends, void *d_out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                       uint64_t *out_unitigs, uint64_t *out_symbol_total, void *hip_stream) {
    return unitigs(bwt, k, min_count, min_edge, false, static_cast<hipStream_t>(hip_stream),
                   {d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total});
}

int msbwt_rle_unitig_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::unitig_info, out); }

// the host call of `nodes` nodes that fills every buffer with `unitigs` unitigs of `symbols` symbols (none of either: the counting call)
int msbwt_unitigs_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t *device_bytes) {
    return unitigs_plan(false, kPlanColumns, total_rows, free_hbm_bytes, nodes, unitigs, symbols, 0, 0, device_bytes);
}

// ---- canonical unitigs: the non-branching paths of the strand-merged k-mer graph ----

int msbwt_rle_enumerate_canonical_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                          uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                          uint64_t *out_unitigs, uint64_t *out_symbol_total) {
    return canonical_unitigs(bwt, k, min_count, min_edge, true, nullptr,
                             {out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total});
}

int msbwt_rle_enumerate_canonical_unitigs_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                                 void *d_out_count_sums, void *d_out_ends, void *d_out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                                 uint64_t *out_unitigs, uint64_t *out_symbol_total, void *hip_stream) {
    return canonical_unitigs(bwt, k, min_count, min_edge, false, static_cast<hipStream_t>(hip_stream),
                             {d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total});
}

int msbwt_rle_canonical_unitig_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::canonical_unitig_info, out); }

// the host call over `classes` classes that fills every buffer with `unitigs` unitigs of `symbols` symbols (none of either: the counting call)
int msbwt_canonical_unitigs_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols, uint64_t *device_bytes) {
    return unitigs_plan(true, kPlanColumns, total_rows, free_hbm_bytes, classes, unitigs, symbols, 0, 0, device_bytes);
}

// ---- unitig graphs: either unitig call with the link table of the compacted graph behind it ----

int msbwt_rle_enumerate_unitig_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                     uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets, uint64_t *out_link_targets,
                                     uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                     uint64_t *out_links) {
    return unitigs(bwt, k, min_count, min_edge, true, nullptr,
                   {out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                    UnitigLinkTable{out_link_offsets, out_link_targets, capacity_links, out_links}});
}

int msbwt_rle_enumerate_unitig_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                            void *d_out_count_sums, void *d_out_ends, void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                            uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                            uint64_t *out_links, void *hip_stream) {
    return unitigs(bwt, k, min_count, min_edge, false, static_cast<hipStream_t>(hip_stream),
                   {d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                    UnitigLinkTable{d_out_link_offsets, d_out_link_targets, capacity_links, out_links}});
}

int msbwt_rle_enumerate_canonical_unitig_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                               uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets, uint64_t *out_link_targets,
                                               uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs,
                                               uint64_t *out_symbol_total, uint64_t *out_links) {
    return canonical_unitigs(bwt, k, min_count, min_edge, true, nullptr,
                             {out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                              UnitigLinkTable{out_link_offsets, out_link_targets, capacity_links, out_links}});
}

int msbwt_rle_enumerate_canonical_unitig_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                                      void *d_out_count_sums, void *d_out_ends, void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                                      uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs,
                                                      uint64_t *out_symbol_total, uint64_t *out_links, void *hip_stream) {
    return canonical_unitigs(bwt, k, min_count, min_edge, false, static_cast<hipStream_t>(hip_stream),
                             {d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                              UnitigLinkTable{d_out_link_offsets, d_out_link_targets, capacity_links, out_links}});
}

// the host call that fills every buffer, the two link arrays included (none of unitigs, symbols and links: the counting call)
int msbwt_unitig_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links, uint64_t *device_bytes) {
    return unitigs_plan(false, kPlanLinks, total_rows, free_hbm_bytes, nodes, unitigs, symbols, links, 0, device_bytes);
}

int msbwt_canonical_unitig_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols, uint64_t links,
                                      uint64_t *device_bytes) {
    return unitigs_plan(true, kPlanLinks, total_rows, free_hbm_bytes, classes, unitigs, symbols, links, 0, device_bytes);
}

// ---- unitig graphs by source: either unitig graph call with the U x S matrix of per-input sums behind the link table ----

int msbwt_rle_enumerate_unitig_graph_by_source(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                               uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets, uint64_t *out_link_targets,
                                               uint64_t *out_source_sums, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                               uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links) {
    return unitigs(bwt, k, min_count, min_edge, true, nullptr,
                   {out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                    UnitigLinkTable{out_link_offsets, out_link_targets, capacity_links, out_links}, UnitigSourceMatrix{out_source_sums}});
}

int msbwt_rle_enumerate_unitig_graph_by_source_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                                      void *d_out_count_sums, void *d_out_ends, void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                                      void *d_out_source_sums, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                                      uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links, void *hip_stream) {
    return unitigs(bwt, k, min_count, min_edge, false, static_cast<hipStream_t>(hip_stream),
                   {d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                    UnitigLinkTable{d_out_link_offsets, d_out_link_targets, capacity_links, out_links}, UnitigSourceMatrix{d_out_source_sums}});
}

int msbwt_rle_enumerate_canonical_unitig_graph_by_source(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols,
                                                         uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags,
                                                         uint64_t *out_link_offsets, uint64_t *out_link_targets, uint64_t *out_source_sums, uint64_t capacity_unitigs,
                                                         uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                                         uint64_t *out_links) {
    return canonical_unitigs(bwt, k, min_count, min_edge, true, nullptr,
                             {out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                              UnitigLinkTable{out_link_offsets, out_link_targets, capacity_links, out_links}, UnitigSourceMatrix{out_source_sums}});
}

int msbwt_rle_enumerate_canonical_unitig_graph_by_source_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols,
                                                                void *d_out_offsets, void *d_out_count_sums, void *d_out_ends, void *d_out_flags,
                                                                void *d_out_link_offsets, void *d_out_link_targets, void *d_out_source_sums, uint64_t capacity_unitigs,
                                                                uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                                                uint64_t *out_links, void *hip_stream) {
    return canonical_unitigs(bwt, k, min_count, min_edge, false, static_cast<hipStream_t>(hip_stream),
                             {d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total,
                              UnitigLinkTable{d_out_link_offsets, d_out_link_targets, capacity_links, out_links}, UnitigSourceMatrix{d_out_source_sums}});
}

// the graph plan of the same kind and, unless it is the counting call, unitig_source_layout with the matrix staged
int msbwt_unitig_graph_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links, size_t n_sources,
                                      uint64_t *device_bytes) {
    return unitigs_plan(false, kPlanSources, total_rows, free_hbm_bytes, nodes, unitigs, symbols, links, n_sources, device_bytes);
}

int msbwt_canonical_unitig_graph_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols, uint64_t links,
                                                size_t n_sources, uint64_t *device_bytes) {
    return unitigs_plan(true, kPlanSources, total_rows, free_hbm_bytes, classes, unitigs, symbols, links, n_sources, device_bytes);
}

}  // extern "C"
