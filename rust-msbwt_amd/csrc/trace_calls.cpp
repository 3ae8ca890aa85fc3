// The trace calls of a loaded index (trace.hpp, canonical_trace.hpp): seed k-mers walked through the k-mer graph or through the
// strand-merged one, each in a host and a device form.  No walk of the index but rounds of the packed search (query.cpp) over the live
// walks of a batch of seeds, in the frame of walk_call.hpp; where the arrays of the call's one block lie is graph_layouts.hpp's.
#include "walk_call.hpp"

#include "canonical_trace.hpp"
#include "graph_layouts.hpp"
#include "trace.hpp"

namespace {

constexpr uint64_t kTracePiece = 1ull << 20;  // the automatic piece
constexpr uint64_t kTraceLimit = 1ull << 40;  // max_steps, and the symbols of all rows, stay below
static_assert(MSBWT_TRACE_INFO_WORDS == 8 && MSBWT_TRACE_RIGHT == kTraceRight && MSBWT_TRACE_LEFT == kTraceLeft && MSBWT_TRACE_UNIQUE == kTraceUnique &&
                  MSBWT_TRACE_UNITIG == kTraceUnitig && MSBWT_TRACE_GREEDY == kTraceGreedy && MSBWT_TRACE_DEAD_END == kTraceDeadEnd && MSBWT_TRACE_BRANCH == kTraceBranch &&
                  MSBWT_TRACE_MERGE == kTraceMerge && MSBWT_TRACE_RETURNED == kTraceReturned && MSBWT_TRACE_TARGET == kTraceTarget &&
                  MSBWT_TRACE_MAX_STEPS == kTraceMaxSteps && MSBWT_TRACE_NOT_A_NODE == kTraceNotANode,
              "the header's constants");
static_assert(MSBWT_CANONICAL_TRACE_INFO_WORDS == MSBWT_TRACE_INFO_WORDS && MSBWT_CANONICAL_TRACE_MIRROR == kCanonicalTraceMirror, "the header's constants");

// The graph a call walks: G, or the strand-merged D -- whose rounds search every edge with its reverse complement and, where a far end
// can be a palindrome below the node threshold (even k, m >= 2), that far end too.  The pieces, the rounds and the guards are one.
struct TraceGraph {
    const char *name;
    bool canonical;
    uint64_t (msbwt_rle::*info)[MSBWT_TRACE_INFO_WORDS];
};
constexpr TraceGraph kPlainGraph{"trace_kmers", false, &msbwt_rle::trace_info}, kCanonicalGraph{"trace_canonical_kmers", true, &msbwt_rle::canonical_trace_info};

bool trace_mode_ok(int mode) { return mode == kTraceUnique || mode == kTraceUnitig || mode == kTraceGreedy; }
bool trace_too_large(uint64_t n, uint64_t max_steps) { return max_steps >= kTraceLimit || (max_steps && n > (kTraceLimit - 1) / max_steps); }
uint64_t trace_piece_walks(uint64_t n, uint64_t piece) { return std::min(n, piece ? piece : kTracePiece); }

// A piece of a host form's wanted column -- `rows` rows of the caller's array from row `first` on -- up to its staged place, or down from it.
int copy_piece(Frame &f, const Column &c, uint64_t first, uint64_t rows, hipMemcpyKind kind) {
    if (!c.out || !c.bytes) return MSBWT_OK;
    char *theirs = static_cast<char *>(c.out) + first * c.bytes;
    const bool up = kind == hipMemcpyHostToDevice;
    HIP_TRY(f.h, hipMemcpyAsync(up ? c.at : theirs, up ? theirs : c.at, rows * c.bytes, kind, f.stream));
    return MSBWT_OK;
}

// Both forms of both calls.  A piece of walks at a time: the seeds become states and round 0's queries; then, round by round, the packed
// search over the live walks' queries and the one kernel that reads its counts (trace.hpp, canonical_trace.hpp), until the live count
// the host reads back is 0 -- after max_steps + 1 rounds at the most.  A host form stages a piece's seeds, targets and outputs in the
// call's block.
int trace_kmers(const TraceGraph &g, const msbwt_rle *bwt, const void *seeds, const void *targets, size_t k, size_t n, uint64_t min_count, uint64_t min_edge, int mode,
                int direction, uint64_t max_steps, bool host, void *out_symbols, void *out_steps, void *out_stops, void *out_edge_sums, void *out_last, void *out_fans,
                hipStream_t stream) {
    Frame f(bwt, g.name, k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = f.open(false, [&]() -> int {
            if (k > 31) return f.refuse(" needs 1 <= k <= 31 (an edge is a packed (k+1)-mer)");
            if (int rc = cut.thresholds(f)) return rc;
            if (!trace_mode_ok(mode)) return f.refuse(": mode is none of MSBWT_TRACE_UNIQUE, _UNITIG, _GREEDY");
            if (direction != kTraceRight && direction != kTraceLeft) return f.refuse(": direction is neither MSBWT_TRACE_RIGHT nor MSBWT_TRACE_LEFT");
            if (n && !seeds) return fail(f.h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer");
            if (trace_too_large(n, max_steps)) return fail(f.h, MSBWT_ERR_TOO_LARGE, f.name + ": max_steps and n x max_steps must stay below 2^40");
            return MSBWT_OK;
        }))
        return rc;
    msbwt_rle *h = f.h;
    uint64_t info[MSBWT_TRACE_INFO_WORDS] = {n, 0, 0, 0, 0, 0, 0, 0};
    const auto close = [&](int rc) {
        info[6] = f.arena.taken;
        std::copy(info, info + MSBWT_TRACE_INFO_WORDS, h->*g.info);
        return rc;
    };
    std::fill(h->*g.info, h->*g.info + MSBWT_TRACE_INFO_WORDS, 0ull);
    if (n == 0) return close(MSBWT_OK);
    const uint64_t mask = (1ull << (2 * k)) - 1;
    TraceCall c{uint32_t(k), mode, direction, cut.m, cut.me, max_steps, 0, n, static_cast<const uint64_t *>(seeds), static_cast<const uint64_t *>(targets),
                static_cast<uint8_t *>(out_symbols), static_cast<uint64_t *>(out_steps), static_cast<uint8_t *>(out_stops), static_cast<uint64_t *>(out_edge_sums),
                static_cast<uint64_t *>(out_last), static_cast<uint8_t *>(out_fans), nullptr, h->d_flags + f.which};
    if (f.empty()) {  // no node at all
        info[7] = n;
        if (host) {
            for (size_t i = 0; i < n; ++i) {
                if (c.steps) c.steps[i] = 0;
                if (c.stops) c.stops[i] = kTraceNotANode;
                if (c.edge_sums) c.edge_sums[i] = 0;
                if (c.last) c.last[i] = c.seeds[i] & mask;
                if (c.fans) c.fans[i] = 0;
            }
            return close(MSBWT_OK);
        }
        HIP_TRY(h, launch_trace_not_nodes(c, f.stream));
        HIP_TRY(h, hipStreamSynchronize(f.stream));
        return close(MSBWT_OK);
    }

    const uint64_t P = trace_piece_walks(n, h->trace_piece);
    // the (k+1)-mers a live walk and later round asks for, and (the node clause) its far ends of length k
    const uint32_t q = g.canonical ? canonical_trace_edge_queries(mode) : trace_queries_per_walk(mode);
    const uint32_t far = g.canonical && k % 2 == 0 && cut.m >= 2 ? canonical_trace_node_queries(mode) : 0;
    const TraceLayout at = (g.canonical ? canonical_trace_layout : trace_layout)(P, max_steps, mode, targets != nullptr, host);
    char *block = nullptr;
    if (int rc = f.take(&block, at.bytes, f.needs(at.bytes, false, "while it runs"), true)) return rc;
    c.counters = in<unsigned long long>(block, at.counters);
    uint64_t *queries = in<uint64_t>(block, at.queries), *counts = in<uint64_t>(block, at.counts);
    const auto search = [&](uint64_t from, size_t len, uint64_t words) {  // queries[from .. from + words) -> counts, at the same place
        info[2] += words;
        return launch_count_2bit(h, queries + from, len, size_t(words), counts + from, f.stream, f.which);
    };
    // A piece's columns.  A host form stages them in the block, and the kernels write every staged column, wanted or not: they are
    // scratch there -- all but the targets, which a call may do without.  A device form's are the caller's own.
    Column inputs[] = {{const_cast<void *>(seeds), 8, P, at.seeds, host}, {const_cast<void *>(targets), 8, P, at.targets}};
    Column outputs[] = {{out_symbols, max_steps, P, at.symbols, host}, {out_steps, 8, P, at.steps, host}, {out_stops, 1, P, at.stops, host},
                        {out_edge_sums, 8, P, at.edge_sums, host}, {out_last, 8, P, at.last, host}, {out_fans, 1, P, at.fans, host}};
    place(f, inputs, block);
    place(f, outputs, block);
    c.seeds = inputs[0].as<const uint64_t>();
    c.targets = inputs[1].as<const uint64_t>();
    c.symbols = outputs[0].as<uint8_t>();
    c.steps = outputs[1].as<uint64_t>();
    c.stops = outputs[2].as<uint8_t>();
    c.edge_sums = outputs[3].as<uint64_t>();
    c.last = outputs[4].as<uint64_t>();
    c.fans = outputs[5].as<uint8_t>();
    for (uint64_t first = 0; first < n; first += P) {
        const uint64_t walks = std::min(P, n - first);
        if (host) {
            c.first = first;
            c.rows = walks;
            for (const Column &col : inputs)
                if (int rc = copy_piece(f, col, first, walks, hipMemcpyHostToDevice)) return rc;
            // a row's tail behind its symbols stays the caller's: the rows go up before they come down
            if (int rc = copy_piece(f, outputs[0], first, walks, hipMemcpyHostToDevice)) return rc;
        }
        TraceWalk *cur = in<TraceWalk>(block, at.states[0]), *other = in<TraceWalk>(block, at.states[1]);
        HIP_TRY(h, hipMemsetAsync(c.counters, 0, kTraceCounterBytes, f.stream));
        if (g.canonical) {  // the seed and its reverse complement, the 8 of its fan, the far end
            HIP_TRY(h, launch_canonical_trace_seed(c, first, walks, cur, queries, f.stream));
            if (int rc = search(0, k, 2 * walks)) return rc;
            if (int rc = search(2 * walks, k + 1, 8 * walks)) return rc;
            if (far)
                if (int rc = search(10 * walks, k, walks)) return rc;
        } else {
            HIP_TRY(h, launch_trace_seed(c, first, walks, cur, queries, f.stream));
            if (int rc = search(0, k, walks)) return rc;
            if (int rc = search(walks, k + 1, 4 * walks)) return rc;
        }
        uint64_t live = walks, left[kTraceCounterWords] = {};
        for (uint64_t round = 0; live && round <= max_steps; ++round) {
            if (round) {
                if (int rc = search(0, k + 1, q * live)) return rc;
                if (far)
                    if (int rc = search(q * walks, k, far * live)) return rc;
            }
            HIP_TRY(h, hipMemsetAsync(c.counters + kTraceLive, 0, 8, f.stream));
            HIP_TRY(h, g.canonical ? launch_canonical_trace_round(c, round == 0, far != 0, walks, live, cur, counts, other, queries, f.stream)
                                   : launch_trace_round(c, round == 0, walks, live, cur, counts, other, queries, f.stream));
            std::swap(cur, other);
            ++info[1];
            if (int rc = read_counters(f, c.counters, left)) return rc;
            if (left[kTraceLive] > live) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": a round left more walks than it took");
            live = left[kTraceLive];
        }
        if (live) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": " + std::to_string(live) + " walks are live after max_steps + 1 rounds");
        info[3] += left[kTraceSteps];
        info[4] = std::max<uint64_t>(info[4], left[kTraceLongest]);
        info[7] += left[kTraceNotNodes];
        ++info[5];
        if (host)
            for (const Column &col : outputs)
                if (int rc = copy_piece(f, col, first, walks, hipMemcpyDeviceToHost)) return rc;
    }
    if (host) return close(status_of(h, f.stream, f.which));  // synchronises
    HIP_TRY(h, hipStreamSynchronize(f.stream));                // (the scratch is freed on return)
    return close(MSBWT_OK);
}

// the one block of a call on an index that holds something: its layout at the piece the call takes
int trace_plan(const TraceGraph &g, uint64_t n, uint64_t max_steps, int mode, int targets, int host, uint64_t piece, uint64_t *device_bytes) {
    if (!trace_mode_ok(mode)) return MSBWT_ERR_INVALID_ARG;
    if (trace_too_large(n, max_steps)) return MSBWT_ERR_TOO_LARGE;
    const auto layout = g.canonical ? canonical_trace_layout : trace_layout;
    if (device_bytes) *device_bytes = n ? layout(trace_piece_walks(n, piece), max_steps, mode, targets != 0, host != 0).bytes : 0;
    return MSBWT_OK;
}

}  // namespace

extern "C" {

int msbwt_rle_trace_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge, int mode,
                          int direction, uint64_t max_steps, uint8_t *out_symbols, uint64_t *out_steps, uint8_t *out_stops, uint64_t *out_edge_sums, uint64_t *out_last,
                          uint8_t *out_fans) {
    return trace_kmers(kPlainGraph, bwt, seeds2bit, targets2bit, k, n, min_count, min_edge, mode, direction, max_steps, true, out_symbols, out_steps, out_stops, out_edge_sums,
                       out_last, out_fans, nullptr);
}

int msbwt_rle_trace_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge,
                                 int mode, int direction, uint64_t max_steps, void *d_out_symbols, void *d_out_steps, void *d_out_stops, void *d_out_edge_sums,
                                 void *d_out_last, void *d_out_fans, void *hip_stream) {
    return trace_kmers(kPlainGraph, bwt, d_seeds2bit, d_targets2bit, k, n, min_count, min_edge, mode, direction, max_steps, false, d_out_symbols, d_out_steps, d_out_stops,
                       d_out_edge_sums, d_out_last, d_out_fans, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_trace_canonical_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge,
                                    int mode, int direction, uint64_t max_steps, uint8_t *out_symbols, uint64_t *out_steps, uint8_t *out_stops, uint64_t *out_edge_sums,
                                    uint64_t *out_last, uint8_t *out_fans) {
    return trace_kmers(kCanonicalGraph, bwt, seeds2bit, targets2bit, k, n, min_count, min_edge, mode, direction, max_steps, true, out_symbols, out_steps, out_stops,
                       out_edge_sums, out_last, out_fans, nullptr);
}

int msbwt_rle_trace_canonical_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit, size_t k, size_t n, uint64_t min_count,
                                           uint64_t min_edge, int mode, int direction, uint64_t max_steps, void *d_out_symbols, void *d_out_steps, void *d_out_stops,
                                           void *d_out_edge_sums, void *d_out_last, void *d_out_fans, void *hip_stream) {
    return trace_kmers(kCanonicalGraph, bwt, d_seeds2bit, d_targets2bit, k, n, min_count, min_edge, mode, direction, max_steps, false, d_out_symbols, d_out_steps,
                       d_out_stops, d_out_edge_sums, d_out_last, d_out_fans, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_trace_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::trace_info, out); }
int msbwt_rle_canonical_trace_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::canonical_trace_info, out); }

int msbwt_rle_set_trace_piece(msbwt_rle *bwt, uint64_t walks) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    return set_locked(bwt, bwt->trace_piece, walks);
}

int msbwt_trace_plan(uint64_t n, uint64_t max_steps, int mode, int targets, int host, uint64_t piece, uint64_t *device_bytes) {
    return trace_plan(kPlainGraph, n, max_steps, mode, targets, host, piece, device_bytes);
}
int msbwt_canonical_trace_plan(uint64_t n, uint64_t max_steps, int mode, int targets, int host, uint64_t piece, uint64_t *device_bytes) {
    return trace_plan(kCanonicalGraph, n, max_steps, mode, targets, host, piece, device_bytes);
}

}  // extern "C"
