// The bridge calls of a loaded index (bridges.hpp): all bounded walks of the k-mer graph between two anchor k-mers, in a host and a
// device form.  No walk of the index but rounds of the packed search (query.cpp) over a frontier of walks that grows as well as shrinks,
// in the frame of walk_call.hpp; where the arrays of the call's one block lie is graph_layouts.hpp's.
#include "walk_call.hpp"

#include "bridges.hpp"
#include "graph_layouts.hpp"

namespace {

constexpr uint64_t kBridgeLimit = 1ull << 40;  // the rows of all pairs, and their symbols, stay below
static_assert(MSBWT_BRIDGE_INFO_WORDS == 8 && MSBWT_BRIDGE_RIGHT == kBridgeRight && MSBWT_BRIDGE_LEFT == kBridgeLeft && MSBWT_BRIDGE_EXHAUSTED == kBridgeExhausted &&
                  MSBWT_BRIDGE_FULL == kBridgeFull && MSBWT_BRIDGE_MAX_STEPS == kBridgeMaxSteps && MSBWT_BRIDGE_TOO_WIDE == kBridgeTooWide &&
                  MSBWT_BRIDGE_NO_SEED == kBridgeNoSeed && MSBWT_BRIDGE_NO_TARGET == kBridgeNoTarget && MSBWT_BRIDGE_MAX_STEPS_CAP == kBridgeMaxStepsCap &&
                  MSBWT_BRIDGE_MAX_LIVE_CAP == kBridgeMaxLiveCap,
              "the header's constants");

bool bridge_too_large(uint64_t n, uint64_t max_steps, uint64_t max_paths, uint64_t max_live) {
    if (max_steps > kBridgeMaxStepsCap || max_live > kBridgeMaxLiveCap || max_paths >= kBridgeLimit) return true;
    if (n && max_paths > (kBridgeLimit - 1) / n) return true;
    return max_steps && n * max_paths > (kBridgeLimit - 1) / max_steps;
}

// A piece of a host form's wanted column -- `rows` rows of the caller's array from row `first` on -- up to its staged place, or down from it.
int copy_piece(Frame &f, const Column &c, uint64_t first, uint64_t rows, hipMemcpyKind kind) {
    if (!c.out || !c.bytes) return MSBWT_OK;
    char *theirs = static_cast<char *>(c.out) + first * c.bytes;
    const bool up = kind == hipMemcpyHostToDevice;
    HIP_TRY(f.h, hipMemcpyAsync(up ? c.at : theirs, up ? theirs : c.at, rows * c.bytes, kind, f.stream));
    return MSBWT_OK;
}

// Both forms.  A piece of pairs at a time: round 0 searches every pair's seed and target at length k and the seed's fan at k + 1; then,
// round by round, the four kernels and the scan between two searches of the frontier (bridges.hpp), until the size of the next level
// the host reads back is 0 -- after max_steps rounds at the most.  A host form stages a piece's seeds, targets and outputs in the block.
int bridge_kmers(const msbwt_rle *bwt, const void *seeds, const void *targets, size_t k, size_t n, uint64_t min_count, uint64_t min_edge, int direction, uint64_t min_steps,
                 uint64_t max_steps, uint64_t max_paths, uint64_t max_live, bool host, void *out_symbols, void *out_lengths, void *out_edge_sums, void *out_found,
                 void *out_stops, void *out_depths, void *out_live, hipStream_t stream) {
    Frame f(bwt, "bridge_kmers", k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = f.open(false, [&]() -> int {
            if (k > 31) return f.refuse(" needs 1 <= k <= 31 (an edge is a packed (k+1)-mer)");
            if (int rc = cut.thresholds(f)) return rc;
            if (direction != kBridgeRight && direction != kBridgeLeft) return f.refuse(": direction is neither MSBWT_BRIDGE_RIGHT nor MSBWT_BRIDGE_LEFT");
            if (n && (!seeds || !targets)) return fail(f.h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer");
            if (max_paths == 0 || max_live == 0) return f.refuse(": max_paths and max_live are at least 1");
            if (min_steps > max_steps) return f.refuse(": min_steps is above max_steps");
            if (bridge_too_large(n, max_steps, max_paths, max_live))
                return fail(f.h, MSBWT_ERR_TOO_LARGE, f.name + ": max_steps is at most 4096, max_live at most 2^24, and n x max_paths x max_steps must stay below 2^40");
            return MSBWT_OK;
        }))
        return rc;
    msbwt_rle *h = f.h;
    uint64_t info[MSBWT_BRIDGE_INFO_WORDS] = {n, 0, 0, 0, 0, 0, 0, 0};
    const auto close = [&](int rc) {
        info[6] = f.arena.taken;
        std::copy(info, info + MSBWT_BRIDGE_INFO_WORDS, h->bridge_info);
        return rc;
    };
    std::fill(h->bridge_info, h->bridge_info + MSBWT_BRIDGE_INFO_WORDS, 0ull);
    if (n == 0) return close(MSBWT_OK);
    BridgeCall c{uint32_t(k), direction, cut.m, cut.me, std::max<uint64_t>(min_steps, 1), max_steps, max_paths, max_live, 0, n, static_cast<const uint64_t *>(seeds),
                 static_cast<const uint64_t *>(targets), static_cast<uint8_t *>(out_symbols), static_cast<uint64_t *>(out_lengths), static_cast<uint64_t *>(out_edge_sums),
                 static_cast<uint64_t *>(out_found), static_cast<uint8_t *>(out_stops), static_cast<uint64_t *>(out_depths), static_cast<uint64_t *>(out_live), nullptr,
                 h->d_flags + f.which};
    if (f.empty()) {  // no node at all
        if (host) {
            if (c.lengths) std::fill(c.lengths, c.lengths + n * max_paths, 0ull);
            if (c.edge_sums) std::fill(c.edge_sums, c.edge_sums + n * max_paths, 0ull);
            for (size_t i = 0; i < n; ++i) {
                if (c.found) c.found[i] = 0;
                if (c.stops) c.stops[i] = kBridgeNoSeed;
                if (c.depths) c.depths[i] = 0;
                if (c.live) c.live[i] = 0;
            }
            return close(MSBWT_OK);
        }
        HIP_TRY(h, launch_bridge_no_seeds(c, f.stream));
        HIP_TRY(h, hipStreamSynchronize(f.stream));
        return close(MSBWT_OK);
    }

    const uint64_t P = bridge_piece_pairs(n, max_live, h->bridge_slots), S = bridge_piece_slots(P, max_live);
    const BridgeLayout at = bridge_layout(P, max_steps, max_paths, max_live, host, scan_scratch_words(S));
    char *block = nullptr;
    if (int rc = f.take(&block, at.bytes, f.needs(at.bytes, false, "while it runs"), true)) return rc;
    c.counters = in<unsigned long long>(block, at.counters);
    BridgePiece p{0, 0, S, bridge_state_words(max_steps), in<unsigned long long>(block, at.table), in<uint64_t>(block, at.weights)};
    uint64_t *queries = in<uint64_t>(block, at.queries), *counts = in<uint64_t>(block, at.counts), *scan = in<uint64_t>(block, at.scan);
    const auto search = [&](uint64_t from, size_t len, uint64_t words) {  // queries[from .. from + words) -> counts, at the same place
        info[2] += words;
        return launch_count_2bit(h, queries + from, len, size_t(words), counts + from, f.stream, f.which);
    };
    // A piece's columns.  A host form stages the wanted ones in the block (their room is there whichever are wanted: the plan does not
    // ask); a device form's are the caller's own.
    const uint64_t row = max_paths * max_steps;
    Column inputs[] = {{const_cast<void *>(seeds), 8, P, at.seeds}, {const_cast<void *>(targets), 8, P, at.targets}};
    Column outputs[] = {{out_symbols, row, P, at.symbols},  {out_lengths, 8 * max_paths, P, at.lengths}, {out_edge_sums, 8 * max_paths, P, at.edge_sums},
                        {out_found, 8, P, at.found},        {out_stops, 1, P, at.stops},                 {out_depths, 8, P, at.depths},
                        {out_live, 8, P, at.live}};
    place(f, inputs, block);
    place(f, outputs, block);
    c.seeds = inputs[0].as<const uint64_t>();
    c.targets = inputs[1].as<const uint64_t>();
    c.symbols = outputs[0].as<uint8_t>();
    c.lengths = outputs[1].as<uint64_t>();
    c.edge_sums = outputs[2].as<uint64_t>();
    c.found = outputs[3].as<uint64_t>();
    c.stops = outputs[4].as<uint8_t>();
    c.depths = outputs[5].as<uint64_t>();
    c.live = outputs[6].as<uint64_t>();
    for (uint64_t first = 0; first < n; first += P) {
        const uint64_t pairs = std::min(P, n - first);
        p.first_pair = first;
        p.pairs = pairs;
        if (host) {
            c.first = first;
            c.rows = pairs;
            for (const Column &col : inputs)
                if (int rc = copy_piece(f, col, first, pairs, hipMemcpyHostToDevice)) return rc;
            // a row's tail behind its symbols stays the caller's: the rows go up before they come down
            if (int rc = copy_piece(f, outputs[0], first, pairs, hipMemcpyHostToDevice)) return rc;
        }
        uint64_t *cur = in<uint64_t>(block, at.states[0]), *other = in<uint64_t>(block, at.states[1]);
        HIP_TRY(h, hipMemsetAsync(c.counters, 0, kBridgeCounterBytes, f.stream));
        HIP_TRY(h, launch_bridge_seed(c, p, cur, queries, f.stream));
        if (int rc = search(0, k, 2 * pairs)) return rc;
        if (int rc = search(2 * pairs, k + 1, 4 * pairs)) return rc;
        HIP_TRY(h, launch_bridge_start(c, p, counts, f.stream));
        ++info[1];
        uint64_t left[kBridgeCounterWords] = {};
        if (int rc = read_counters(f, c.counters, left)) return rc;
        uint64_t live = left[kBridgeAlive] ? pairs : 0;  // round 1 goes over every pair's state; one that stopped has no child
        info[7] = std::max(info[7], pairs);
        for (uint64_t round = 1; live && round <= max_steps; ++round) {
            if (round > 1)
                if (int rc = search(0, k + 1, 4 * live)) return rc;
            const uint64_t *fan_counts = round == 1 ? counts + 2 * pairs : counts;
            HIP_TRY(h, launch_bridge_decide(c, p, round, live, cur, fan_counts, f.stream));
            HIP_TRY(h, exclusive_scan(p.weights, live, scan, f.stream));
            HIP_TRY(h, launch_bridge_scatter(c, p, round, live, cur, fan_counts, other, queries, f.stream));
            std::swap(cur, other);
            ++info[1];
            if (int rc = read_counters(f, c.counters, left)) return rc;
            if (left[kBridgeLive] > S) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": a round left more walks than the frontier holds");
            live = left[kBridgeLive];
            info[7] = std::max(info[7], live);
        }
        if (live) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": " + std::to_string(live) + " walks are live after max_steps rounds");
        info[3] += left[kBridgeExpanded];
        info[4] += left[kBridgeFound];
        ++info[5];
        if (host)
            for (const Column &col : outputs)
                if (int rc = copy_piece(f, col, first, pairs, hipMemcpyDeviceToHost)) return rc;
    }
    if (host) return close(status_of(h, f.stream, f.which));  // synchronises
    HIP_TRY(h, hipStreamSynchronize(f.stream));                // (the scratch is freed on return)
    return close(MSBWT_OK);
}

}  // namespace

extern "C" {

int msbwt_rle_bridge_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge,
                           int direction, uint64_t min_steps, uint64_t max_steps, uint64_t max_paths, uint64_t max_live, uint8_t *out_symbols, uint64_t *out_lengths,
                           uint64_t *out_edge_sums, uint64_t *out_found, uint8_t *out_stops, uint64_t *out_depths, uint64_t *out_live) {
    return bridge_kmers(bwt, seeds2bit, targets2bit, k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, true, out_symbols, out_lengths,
                        out_edge_sums, out_found, out_stops, out_depths, out_live, nullptr);
}

int msbwt_rle_bridge_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge,
                                  int direction, uint64_t min_steps, uint64_t max_steps, uint64_t max_paths, uint64_t max_live, void *d_out_symbols, void *d_out_lengths,
                                  void *d_out_edge_sums, void *d_out_found, void *d_out_stops, void *d_out_depths, void *d_out_live, void *hip_stream) {
    return bridge_kmers(bwt, d_seeds2bit, d_targets2bit, k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, false, d_out_symbols,
                        d_out_lengths, d_out_edge_sums, d_out_found, d_out_stops, d_out_depths, d_out_live, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_bridge_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::bridge_info, out); }

int msbwt_rle_set_bridge_slots(msbwt_rle *bwt, uint64_t slots) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    if (slots > kBridgeSlotsCap) {
        std::lock_guard<std::mutex> lock(bwt->mu);
        return fail(bwt, MSBWT_ERR_INVALID_ARG, "the frontier of a bridge call's piece is at most 2^28 slots (0 = automatic)");
    }
    return set_locked(bwt, bwt->bridge_slots, slots);
}

// the one block of a call on an index that holds something: its layout at the piece the call takes
int msbwt_bridge_plan(uint64_t n, uint64_t max_steps, uint64_t max_paths, uint64_t max_live, int host, uint64_t slots, uint64_t *device_bytes) {
    if (max_paths == 0 || max_live == 0 || slots > kBridgeSlotsCap) return MSBWT_ERR_INVALID_ARG;
    if (bridge_too_large(n, max_steps, max_paths, max_live)) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) {
        const uint64_t P = bridge_piece_pairs(n, max_live, slots);
        *device_bytes = n ? bridge_layout(P, max_steps, max_paths, max_live, host != 0, scan_scratch_words(bridge_piece_slots(P, max_live))).bytes : 0;
    }
    return MSBWT_OK;
}

}  // extern "C"
