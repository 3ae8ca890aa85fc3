// The read-overlap calls of a loaded index (overlaps.hpp): msbwt_rle_read_overlaps in a host and a device form, its info words, its
// piece and its plan.  The queries of a call go a piece at a time through one kernel, twice where records are wanted: pass A for the
// per-query outputs and the record counts, a scan, pass B for the records at their places, the running base carried from piece to
// piece.  The skeleton is handle.hpp's Call; Arena, Clock and the small things are walk_call.hpp's.
#include "walk_call.hpp"

#include "overlaps.hpp"

namespace {

static_assert(MSBWT_OVERLAP_INFO_WORDS == 13 && MSBWT_OVERLAP_END == kOverlapEnd && MSBWT_OVERLAP_EMPTY == kOverlapEmpty && MSBWT_OVERLAP_BAD_SYMBOL == kOverlapBadSymbol,
              "the header's constants");

// A call: the handle locked, the guards answered, the device bound, the stream chosen, the clock running, the scratch freed with it.
struct OverlapFrame {
    Call c;
    msbwt_rle *const h;
    const std::string name = "read_overlaps";
    const bool host;
    hipStream_t stream;
    const int which;
    Clock clock;
    Arena arena;
    uint64_t info[MSBWT_OVERLAP_INFO_WORDS] = {};

    OverlapFrame(const msbwt_rle *bwt, bool host, hipStream_t stream) : c(bwt), h(c.h), host(host), stream(stream), which(host ? kHostFlags : kDeviceFlags) {}

    // no handle, no index, the call's own arguments -- args() refuses or returns MSBWT_OK --, the device
    template <class Args>
    int open(Args &&args) {
        if (!h) return MSBWT_ERR_INVALID_ARG;
        if (int rc = c.loaded()) return rc;
        if (int rc = args()) return rc;
        if (int rc = c.bind()) return rc;
        if (int rc = ensure_runtime(h)) return rc;
        if (host) stream = h->stream;
        clock = Clock{};
        std::fill(h->overlap_info, h->overlap_info + MSBWT_OVERLAP_INFO_WORDS, 0ull);
        return MSBWT_OK;
    }
    int refuse(const std::string &why) const { return fail(h, MSBWT_ERR_INVALID_ARG, name + why); }
    template <class T>
    int take(T **p, uint64_t bytes) {
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
        if (free_bytes < bytes || arena.take(p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, name + ": " + std::to_string(bytes) + " bytes of HBM needed while it runs");
        }
        return MSBWT_OK;
    }
    // the counters of the searches launched since they were zeroed (synchronises)
    int read(const unsigned long long *d_counters, uint64_t (&c8)[kOverlapCounterWords]) {
        HIP_TRY(h, hipMemcpyAsync(c8, d_counters, sizeof c8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        return MSBWT_OK;
    }
    int close(int rc) {
        info[10] = clock.us();
        std::copy(info, info + MSBWT_OVERLAP_INFO_WORDS, h->overlap_info);
        return rc;
    }
    // a host form ends on the flags its kernels left (synchronises); a device form on its stream drained
    int finish() {
        if (host) return close(status_of(h, stream, which));
        HIP_TRY(h, hipStreamSynchronize(stream));
        return close(MSBWT_OK);
    }
};

bool overlap_too_large(uint64_t n) { return n >= kOverlapLimit; }

// Both forms of msbwt_rle_read_overlaps.  A host form stages a piece's queries and per-query outputs in the call's block and a piece's
// record columns in a block of their own, taken once the piece's records are counted; a device form's arrays are the caller's own.
int read_overlaps(const msbwt_rle *bwt, const uint8_t *reads, const uint64_t *offsets, size_t n, uint64_t m, uint64_t M, int strand, bool host, uint64_t *out_offsets,
                  uint64_t *out_lengths, uint64_t *out_first, uint64_t *out_counts, uint64_t capacity, uint64_t *out_total, uint64_t *out_matched, uint64_t *out_edges,
                  uint8_t *out_stops, hipStream_t stream) {
    OverlapFrame f(bwt, host, stream);
    const bool some = out_lengths || out_first || out_counts, fill = out_lengths && out_first && out_counts;
    if (int rc = f.open([&]() -> int {
            if ((n && (!reads || !offsets)) || !out_total) return fail(f.h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer");
            if (m == 0) return f.refuse(" needs min_overlap >= 1");
            if (strand != 0 && strand != 1) return f.refuse(": strand is 0 (as given) or 1 (the reverse complement)");
            if (some != fill) return f.refuse(": the record columns come all three or not at all");
            if (overlap_too_large(n)) return fail(f.h, MSBWT_ERR_TOO_LARGE, f.name + ": n and the symbols of all queries must stay below 2^40");
            if (host) {
                for (size_t i = 0; i < n; ++i)
                    if (offsets[i + 1] < offsets[i]) return fail(f.h, MSBWT_ERR_INVALID_RANGE, f.name + ": read_offsets decrease behind query " + std::to_string(i));
                if (n && offsets[n] - offsets[0] >= kOverlapLimit) return fail(f.h, MSBWT_ERR_TOO_LARGE, f.name + ": n and the symbols of all queries must stay below 2^40");
            }
            return MSBWT_OK;
        }))
        return rc;
    msbwt_rle *h = f.h;
    *out_total = 0;
    f.info[0] = n;
    const auto zeros = [&](void *p, int byte, uint64_t bytes) -> int {
        if (!p || !bytes) return MSBWT_OK;
        if (host) {
            std::fill(static_cast<uint8_t *>(p), static_cast<uint8_t *>(p) + bytes, uint8_t(byte));
        } else {
            HIP_TRY(h, hipMemsetAsync(p, byte, bytes, f.stream));
        }
        return MSBWT_OK;
    };
    if (n == 0 || h->totals.total == 0) {  // no query, or an index of no rows: every query EMPTY, nothing allocated
        if (int rc = zeros(out_offsets, 0, 8 * (uint64_t(n) + 1))) return rc;
        if (int rc = zeros(out_matched, 0, 8 * uint64_t(n))) return rc;
        if (int rc = zeros(out_edges, 0, 8 * uint64_t(n))) return rc;
        if (int rc = zeros(out_stops, kOverlapEmpty, n)) return rc;
        f.info[5] = n;
        if (!host) HIP_TRY(h, hipStreamSynchronize(f.stream));
        return f.close(MSBWT_OK);
    }

    const uint64_t P = overlap_piece_queries(n, h->overlap_piece);
    uint64_t piece_symbols = 0;
    if (host)
        for (uint64_t first = 0; first < n; first += P) piece_symbols = std::max(piece_symbols, offsets[std::min<uint64_t>(first + P, n)] - offsets[first]);
    const OverlapLayout at = overlap_layout(P, host, piece_symbols, scan_scratch_words(P + 1));
    char *block = nullptr;
    if (int rc = f.take(&block, at.bytes)) return rc;
    f.info[9] = at.bytes;
    f.info[11] = piece_symbols;
    unsigned long long *counters = in<unsigned long long>(block, at.counters);
    uint64_t *counts = in<uint64_t>(block, at.counts);
    HIP_TRY(h, hipMemsetAsync(counters, 0, kOverlapCounterBytes, f.stream));

    OverlapCall k{};
    k.blocks = h->d_blocks;
    k.overflow = h->d_overflow;
    k.format = h->block_format == kBlocksRuns ? 1u : 0u;
    k.total = h->totals.total;
    for (int s = 0; s < kAlphabet; ++s) k.start[s] = h->totals.start_index[s];
    k.start[kAlphabet] = h->totals.total;
    k.min_overlap = m;
    k.max_overlap = M;
    k.strand = uint32_t(strand);
    k.counters = counters;
    k.flags = h->d_flags + f.which;

    uint64_t c8[kOverlapCounterWords] = {};
    uint64_t base = 0, pieces = 0, staged_records = 0;
    bool short_of = false;  // the capacity ran out: the pieces from there on are counted only
    for (uint64_t first = 0; first < n; first += P, ++pieces) {
        const uint64_t q = std::min<uint64_t>(P, n - first);
        if (host) {
            const uint64_t *off = offsets + first;
            HIP_TRY(h, hipMemcpyAsync(block + at.in_offsets, off, (q + 1) * 8, hipMemcpyHostToDevice, f.stream));
            if (off[q] > off[0]) HIP_TRY(h, hipMemcpyAsync(block + at.symbols, reads + off[0], off[q] - off[0], hipMemcpyHostToDevice, f.stream));
            k.offsets = in<const uint64_t>(block, at.in_offsets);
            k.symbols = in<const uint8_t>(block, at.symbols);
            k.origin = off[0];
            k.trips = 0;
            for (uint64_t i = 0; i < q; ++i) k.trips = std::max(k.trips, M ? std::min(off[i + 1] - off[i], M) : off[i + 1] - off[i]);
        } else {  // the offsets are the device's: the largest E of the piece by a kernel of its own
            k.offsets = offsets + first;
            k.symbols = reads;
            k.origin = 0;
            HIP_TRY(h, launch_overlap_prepare(k.offsets, q, M, counters, k.flags, f.stream));
            if (int rc = f.read(counters, c8)) return rc;
            k.trips = c8[kOverlapMaxE];  // (of the pieces so far: no less than this one's)
        }
        k.n = q;
        // pass A: the per-query outputs and the record counts
        k.rec_counts = counts;
        k.matched = host ? in<uint64_t>(block, at.matched) : out_matched ? out_matched + first : nullptr;
        k.edges = host ? in<uint64_t>(block, at.edges) : out_edges ? out_edges + first : nullptr;
        k.stops = host ? in<uint8_t>(block, at.stops) : out_stops ? out_stops + first : nullptr;
        k.rec_offsets = nullptr;
        k.lengths = k.first = k.counts = nullptr;
        HIP_TRY(h, launch_overlaps(k, f.stream));
        HIP_TRY(h, hipMemsetAsync(counts + q, 0, 8, f.stream));
        HIP_TRY(h, exclusive_scan(counts, q + 1, in<uint64_t>(block, at.scan), f.stream));
        if (out_offsets) HIP_TRY(h, launch_overlap_offsets(counts, q + 1, base, host ? in<uint64_t>(block, at.out_offsets) : out_offsets + first, f.stream));
        if (int rc = f.read(counters, c8)) return rc;  // (synchronises: the base of the next piece)
        const uint64_t upto = c8[kOverlapRecords];
        if (upto < base) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": a piece's records do not add up");
        const uint64_t records = upto - base;
        if (host) {
            if (out_offsets) HIP_TRY(h, hipMemcpyAsync(out_offsets + first, block + at.out_offsets, (q + 1) * 8, hipMemcpyDeviceToHost, f.stream));
            if (out_matched) HIP_TRY(h, hipMemcpyAsync(out_matched + first, block + at.matched, q * 8, hipMemcpyDeviceToHost, f.stream));
            if (out_edges) HIP_TRY(h, hipMemcpyAsync(out_edges + first, block + at.edges, q * 8, hipMemcpyDeviceToHost, f.stream));
            if (out_stops) HIP_TRY(h, hipMemcpyAsync(out_stops + first, block + at.stops, q, hipMemcpyDeviceToHost, f.stream));
        }
        if (fill && upto > capacity) short_of = true;
        if (fill && !short_of && records) {  // pass B: the search again, every record at its place
            k.rec_counts = nullptr;
            k.matched = k.edges = nullptr;
            k.stops = nullptr;
            k.rec_offsets = counts;
            char *columns = nullptr;
            const uint64_t column = overlap_pad(8 * records);
            if (host) {
                if (int rc = f.take(&columns, overlap_column_bytes(records))) return rc;
                staged_records = std::max(staged_records, records);
                k.base = 0;
                k.capacity = records;
                k.lengths = in<uint64_t>(columns, 0);
                k.first = in<uint64_t>(columns, column);
                k.counts = in<uint64_t>(columns, 2 * column);
            } else {
                k.base = base;
                k.capacity = capacity;
                k.lengths = out_lengths;
                k.first = out_first;
                k.counts = out_counts;
            }
            HIP_TRY(h, launch_overlaps(k, f.stream));
            if (host) {
                HIP_TRY(h, hipMemcpyAsync(out_lengths + base, k.lengths, records * 8, hipMemcpyDeviceToHost, f.stream));
                HIP_TRY(h, hipMemcpyAsync(out_first + base, k.first, records * 8, hipMemcpyDeviceToHost, f.stream));
                HIP_TRY(h, hipMemcpyAsync(out_counts + base, k.counts, records * 8, hipMemcpyDeviceToHost, f.stream));
                HIP_TRY(h, hipStreamSynchronize(f.stream));
                f.arena.give_back(columns);
            }
        }
        base = upto;
    }
    if (int rc = f.read(counters, c8)) return rc;
    *out_total = c8[kOverlapRecords];
    f.info[1] = c8[kOverlapSymbols];
    f.info[2] = c8[kOverlapRecords];
    f.info[3] = c8[kOverlapEdges];
    f.info[4] = c8[kOverlapEnds];
    f.info[5] = c8[kOverlapEmpties];
    f.info[6] = c8[kOverlapBads];
    f.info[7] = c8[kOverlapLines];
    f.info[8] = pieces;
    f.info[9] = at.bytes + overlap_column_bytes(staged_records);
    f.info[12] = staged_records;
    if (short_of) {
        const int flagged = f.finish();  // (a device form's bad symbol stays in its flags)
        if (flagged) return flagged;
        return f.refuse(": capacity_records " + std::to_string(capacity) + " is less than the R = " + std::to_string(*out_total) + " records of the queries");
    }
    return f.finish();
}

}  // namespace

extern "C" {

int msbwt_rle_read_overlaps(const msbwt_rle *bwt, const uint8_t *reads, const uint64_t *read_offsets, size_t n, uint64_t min_overlap, uint64_t max_overlap, int strand,
                            uint64_t *out_offsets, uint64_t *out_lengths, uint64_t *out_first, uint64_t *out_counts, uint64_t capacity_records, uint64_t *out_record_total,
                            uint64_t *out_matched, uint64_t *out_edges, uint8_t *out_stops) {
    return read_overlaps(bwt, reads, read_offsets, n, min_overlap, max_overlap, strand, true, out_offsets, out_lengths, out_first, out_counts, capacity_records,
                         out_record_total, out_matched, out_edges, out_stops, nullptr);
}

int msbwt_rle_read_overlaps_device(const msbwt_rle *bwt, const void *d_reads, const void *d_read_offsets, size_t n, uint64_t min_overlap, uint64_t max_overlap, int strand,
                                   void *d_out_offsets, void *d_out_lengths, void *d_out_first, void *d_out_counts, uint64_t capacity_records, uint64_t *out_record_total,
                                   void *d_out_matched, void *d_out_edges, void *d_out_stops, void *hip_stream) {
    return read_overlaps(bwt, static_cast<const uint8_t *>(d_reads), static_cast<const uint64_t *>(d_read_offsets), n, min_overlap, max_overlap, strand, false,
                         static_cast<uint64_t *>(d_out_offsets), static_cast<uint64_t *>(d_out_lengths), static_cast<uint64_t *>(d_out_first),
                         static_cast<uint64_t *>(d_out_counts), capacity_records, out_record_total, static_cast<uint64_t *>(d_out_matched),
                         static_cast<uint64_t *>(d_out_edges), static_cast<uint8_t *>(d_out_stops), static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_overlap_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::overlap_info, out); }

int msbwt_rle_set_overlap_piece(msbwt_rle *bwt, uint64_t queries) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    if (queries > kOverlapMaxPiece) {
        std::lock_guard<std::mutex> lock(bwt->mu);
        return fail(bwt, MSBWT_ERR_INVALID_ARG, "a piece of overlap queries is at most 2^28 queries (0 = automatic)");
    }
    return set_locked(bwt, bwt->overlap_piece, queries);
}

int msbwt_overlap_plan(uint64_t n, int host, uint64_t piece, uint64_t piece_symbols, uint64_t piece_records, uint64_t *device_bytes) {
    if (piece > kOverlapMaxPiece) return MSBWT_ERR_INVALID_ARG;
    if (overlap_too_large(n) || piece_symbols >= kOverlapLimit || piece_records >= kOverlapLimit) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) {
        const uint64_t P = overlap_piece_queries(n, piece);
        *device_bytes = n ? overlap_layout(P, host != 0, host ? piece_symbols : 0, scan_scratch_words(P + 1)).bytes + (host ? overlap_column_bytes(piece_records) : 0) : 0;
    }
    return MSBWT_OK;
}

}  // extern "C"
