// The left-walk calls of a loaded index (left_walk.hpp): rows walked back through the text -- msbwt_rle_walk_rows, locate when no symbols
// are wanted -- and reads extracted in reading order, each in a host and a device form.  The walks of a call go a piece at a time
// through one kernel; where the arrays of the call's one block lie is left_walk.hpp's.  The skeleton is handle.hpp's Call (the k-mer
// calls' Frame is a ladder about k); Arena, Clock, Column and the small things are walk_call.hpp's.
#include "walk_call.hpp"

#include "left_walk.hpp"

namespace {

static_assert(MSBWT_WALK_INFO_WORDS == 8 && MSBWT_WALK_DOLLAR == kWalkDollar && MSBWT_WALK_MAX_STEPS == kWalkMaxSteps && MSBWT_WALK_BAD_ROW == kWalkBadRow,
              "the header's constants");

// A call: the handle locked, the guards answered, the device bound, the stream chosen, the clock running, the scratch freed with it.
struct WalkFrame {
    Call c;
    msbwt_rle *const h;
    const std::string name;
    const bool host;
    hipStream_t stream;
    const int which;
    Clock clock;
    Arena arena;
    uint64_t info[MSBWT_WALK_INFO_WORDS] = {};

    WalkFrame(const msbwt_rle *bwt, const char *name, bool host, hipStream_t stream)
        : c(bwt), h(c.h), name(name), host(host), stream(stream), which(host ? kHostFlags : kDeviceFlags) {}

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
        std::fill(h->walk_info, h->walk_info + MSBWT_WALK_INFO_WORDS, 0ull);
        return MSBWT_OK;
    }
    int null_pointer() const { return fail(h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer"); }
    int too_large(const char *steps) const { return fail(h, MSBWT_ERR_TOO_LARGE, name + ": " + steps + " and n x " + steps + " must stay below 2^40"); }
    int take(char **block, uint64_t bytes) {
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
        if (free_bytes < bytes || arena.take(block, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, name + ": " + std::to_string(bytes) + " bytes of HBM needed while it runs");
        }
        return MSBWT_OK;
    }
    // the counters of the walks launched since they were zeroed, into the info words (synchronises)
    int tally(const unsigned long long *d_counters, uint64_t walks, uint64_t pieces) {
        uint64_t c4[kWalkCounterWords] = {};
        HIP_TRY(h, hipMemcpyAsync(c4, d_counters, sizeof c4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        info[0] = walks;
        info[1] = c4[kWalkSteps];
        info[2] = c4[kWalkDollars];
        info[3] = c4[kWalkMaxed];
        info[4] = c4[kWalkBad];
        info[5] = pieces;
        return MSBWT_OK;
    }
    int close(int rc) {
        info[6] = arena.taken;
        info[7] = clock.us();
        std::copy(info, info + MSBWT_WALK_INFO_WORDS, h->walk_info);
        return rc;
    }
    // a host form ends on the flags its kernels left (synchronises); a device form on its stream drained: the scratch goes with the frame
    int finish() {
        if (host) return close(status_of(h, stream, which));
        HIP_TRY(h, hipStreamSynchronize(stream));
        return close(MSBWT_OK);
    }
    LeftWalkCall kernel_call(uint64_t max_steps, unsigned long long *counters) const {
        LeftWalkCall k{};
        k.blocks = h->d_blocks;
        k.overflow = h->d_overflow;
        k.format = h->block_format == kBlocksRuns ? 1u : 0u;
        k.total = h->totals.total;
        k.dollars = h->totals.start_index[1];
        k.max_steps = max_steps;
        k.stride = max_steps;
        k.counters = counters;
        k.flags = h->d_flags + which;
        return k;
    }
};

// A piece of a host form's wanted column -- `rows` rows of the caller's array from row `first` on -- up to its staged place, or down from it.
int copy_piece(WalkFrame &f, const Column &c, uint64_t first, uint64_t rows, hipMemcpyKind kind) {
    if (!c.out || !c.bytes || !rows) return MSBWT_OK;
    char *theirs = static_cast<char *>(c.out) + first * c.bytes;
    const bool up = kind == hipMemcpyHostToDevice;
    HIP_TRY(f.h, hipMemcpyAsync(up ? c.at : theirs, up ? theirs : c.at, rows * c.bytes, kind, f.stream));
    return MSBWT_OK;
}

// Both forms of msbwt_rle_walk_rows.  A host form stages a piece's rows and outputs in the call's block -- the kernel writes every
// staged output, wanted or not; only the rows of symbols are staged on demand --, a device form's arrays are the caller's own.
int walk_rows(const msbwt_rle *bwt, const void *rows, size_t n, uint64_t max_steps, bool host, void *out_symbols, void *out_steps, void *out_stops, void *out_last,
              void *out_reads, hipStream_t stream) {
    WalkFrame f(bwt, "walk_rows", host, stream);
    if (int rc = f.open([&]() -> int {
            if (n && !rows) return f.null_pointer();
            if (walk_too_large(n, max_steps)) return f.too_large("max_steps");
            return MSBWT_OK;
        }))
        return rc;
    msbwt_rle *h = f.h;
    if (n == 0 || h->totals.total == 0) return f.close(MSBWT_OK);
    const uint64_t P = walk_piece_walks(n, h->walk_piece);
    const WalkLayout at = walk_layout(P, max_steps, out_symbols != nullptr, host);
    char *block = nullptr;
    if (int rc = f.take(&block, at.bytes)) return rc;
    unsigned long long *counters = in<unsigned long long>(block, at.counters);
    HIP_TRY(h, hipMemsetAsync(counters, 0, kWalkCounterBytes, f.stream));
    LeftWalkCall k = f.kernel_call(max_steps, counters);
    Column input{const_cast<void *>(rows), 8, P, at.rows, host};
    Column outputs[] = {{out_symbols, max_steps, P, at.symbols}, {out_steps, 8, P, at.steps, host}, {out_stops, 1, P, at.stops, host},
                        {out_last, 8, P, at.last, host}, {out_reads, 8, P, at.reads, host}};
    uint64_t pieces = 0;
    for (uint64_t first = 0; first < n; first += P, ++pieces) {
        const uint64_t walks = std::min<uint64_t>(P, n - first);
        // where this piece's arrays are: staged at their offsets, or `first` rows into the caller's own
        const auto at_piece = [&](const Column &c) -> void * {
            if (host) return c.scratch || c.out ? block + c.offset : nullptr;
            return c.out ? static_cast<char *>(c.out) + first * c.bytes : nullptr;
        };
        input.at = at_piece(input);
        for (Column &c : outputs) c.at = at_piece(c);
        if (host) {
            if (int rc = copy_piece(f, input, first, walks, hipMemcpyHostToDevice)) return rc;
            // a row's tail behind its symbols stays the caller's: the rows go up before they come down
            if (int rc = copy_piece(f, outputs[0], first, walks, hipMemcpyHostToDevice)) return rc;
        }
        k.rows = input.as<const uint64_t>();
        k.n = walks;
        k.symbols = outputs[0].as<uint8_t>();
        k.steps = outputs[1].as<uint64_t>();
        k.stops = outputs[2].as<uint8_t>();
        k.last = outputs[3].as<uint64_t>();
        k.reads = outputs[4].as<uint64_t>();
        HIP_TRY(h, launch_left_walk(k, f.stream));
        if (host)
            for (const Column &c : outputs)
                if (int rc = copy_piece(f, c, first, walks, hipMemcpyDeviceToHost)) return rc;
    }
    if (int rc = f.tally(counters, n, pieces)) return rc;
    return f.finish();
}

// Both forms of msbwt_rle_extract_reads.  One pass over the n reads, a piece at a time: the walk (ids as rows, max_len steps) leaves
// the lengths and, when symbols are copied, the walk-order rows; the lengths are scanned in place; the reverse kernel puts the piece's
// symbols and offsets where they belong; the counters, read back a piece, carry the base to the next.  A capacity that S may exceed
// is settled by a pass without copies first.
int extract_reads(const msbwt_rle *bwt, const void *read_ids, uint64_t first_read, size_t n, uint64_t max_len, bool host, void *out_symbols, void *out_offsets,
                  uint64_t capacity, uint64_t *out_total, uint64_t *out_truncated, hipStream_t stream) {
    WalkFrame f(bwt, "extract_reads", host, stream);
    if (int rc = f.open([&]() -> int {
            if (max_len == 0) return fail(f.h, MSBWT_ERR_INVALID_ARG, f.name + " needs max_len >= 1");
            if (!out_total) return fail(f.h, MSBWT_ERR_INVALID_ARG, "null pointer");
            if (walk_too_large(n, max_len)) return f.too_large("max_len");
            const uint64_t reads = f.h->totals.start_index[1];
            const auto refuse = [&](uint64_t id) {
                return fail(f.h, MSBWT_ERR_INVALID_RANGE, f.name + ": read " + std::to_string(id) + " is not below the " + std::to_string(reads) + " reads of the index");
            };
            if (!read_ids && n && (first_read >= reads || n > reads - first_read)) return refuse(first_read >= reads ? first_read : reads);
            if (read_ids && host)
                for (size_t i = 0; i < n; ++i)
                    if (static_cast<const uint64_t *>(read_ids)[i] >= reads) return refuse(static_cast<const uint64_t *>(read_ids)[i]);
            return MSBWT_OK;
        }))
        return rc;
    msbwt_rle *h = f.h;
    *out_total = 0;
    if (out_truncated) *out_truncated = 0;
    if (n == 0) {
        if (out_offsets && host) *static_cast<uint64_t *>(out_offsets) = 0;
        if (out_offsets && !host) {
            HIP_TRY(h, hipMemsetAsync(out_offsets, 0, 8, f.stream));
            HIP_TRY(h, hipStreamSynchronize(f.stream));
        }
        return f.close(MSBWT_OK);
    }
    const bool want = out_symbols != nullptr;
    const uint64_t P = walk_piece_walks(n, h->walk_piece);
    const ExtractLayout at = extract_layout(P, max_len, read_ids != nullptr, want, out_offsets != nullptr, host, scan_scratch_words(P + 1));
    char *block = nullptr;
    if (int rc = f.take(&block, at.bytes)) return rc;
    unsigned long long *counters = in<unsigned long long>(block, at.counters);
    uint64_t *lengths = in<uint64_t>(block, at.lengths);
    LeftWalkCall k = f.kernel_call(max_len, counters);
    k.ids = true;
    k.steps = lengths;

    uint64_t launched = 0;  // pieces, of both passes where there are two: the info word tells one walk from two
    const auto pass = [&](bool copy, bool offsets) -> int {
        HIP_TRY(h, hipMemsetAsync(counters, 0, kWalkCounterBytes, f.stream));
        uint64_t base = 0;
        for (uint64_t first = 0; first < n; first += P) {
            const uint64_t walks = std::min<uint64_t>(P, n - first);
            if (read_ids && host) {
                HIP_TRY(h, hipMemcpyAsync(block + at.ids, static_cast<const uint64_t *>(read_ids) + first, walks * 8, hipMemcpyHostToDevice, f.stream));
                k.rows = in<const uint64_t>(block, at.ids);
            } else {
                k.rows = read_ids ? static_cast<const uint64_t *>(read_ids) + first : nullptr;
            }
            k.first_row = first_read + first;
            k.n = walks;
            k.symbols = copy ? in<uint8_t>(block, at.rows) : nullptr;
            HIP_TRY(h, launch_left_walk(k, f.stream));
            const bool place = copy || offsets;  // (a pass for the lengths alone needs the counters only)
            if (place) {
                HIP_TRY(h, hipMemsetAsync(lengths + walks, 0, 8, f.stream));
                HIP_TRY(h, exclusive_scan(lengths, walks + 1, in<uint64_t>(block, at.scan), f.stream));
            }
            // the piece's symbols go to [base, base + its total): staged from 0 on, or straight into the caller's array
            uint8_t *symbols_at = !copy ? nullptr : host ? in<uint8_t>(block, at.symbols) : static_cast<uint8_t *>(out_symbols) + base;
            uint64_t *offsets_at = !offsets ? nullptr : host ? in<uint64_t>(block, at.offsets) : static_cast<uint64_t *>(out_offsets) + first;
            const uint64_t room = host ? walks * max_len : capacity - std::min(base, capacity);
            if (place) HIP_TRY(h, launch_left_walk_reverse(k.symbols, max_len, lengths, walks, base, symbols_at, room, offsets_at, k.flags, f.stream));
            if (int rc = f.tally(counters, n, ++launched)) return rc;  // (synchronises: the base of the next piece)
            const uint64_t upto = f.info[1];
            if (upto < base || upto - base > walks * max_len) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": a piece's lengths do not add up");
            if (host && copy) {
                if (upto > capacity) return fail(h, MSBWT_ERR_INTERNAL, f.name + ": the symbols outgrew the capacity they were measured for");
                HIP_TRY(h, hipMemcpyAsync(static_cast<uint8_t *>(out_symbols) + base, symbols_at, upto - base, hipMemcpyDeviceToHost, f.stream));
            }
            if (host && offsets) HIP_TRY(h, hipMemcpyAsync(static_cast<uint64_t *>(out_offsets) + first, offsets_at, (walks + 1) * 8, hipMemcpyDeviceToHost, f.stream));
            base = upto;
        }
        return MSBWT_OK;
    };
    const auto report = [&] {
        *out_total = f.info[1];
        if (out_truncated) *out_truncated = f.info[3];
    };
    if (want && capacity / max_len < n) {  // S may exceed the capacity: the lengths first, nothing touched
        if (int rc = pass(false, false)) return rc;
        report();
        if (f.info[1] > capacity) {
            const int flagged = f.finish();  // (a device form's bad id stays in its flags)
            if (flagged) return flagged;
            return fail(h, MSBWT_ERR_INVALID_ARG, f.name + ": capacity_symbols " + std::to_string(capacity) + " is less than the S = " + std::to_string(f.info[1]) +
                                                      " symbols of the reads");
        }
    }
    if (int rc = pass(want, out_offsets != nullptr)) return rc;
    report();
    return f.finish();
}

}  // namespace

extern "C" {

int msbwt_rle_walk_rows(const msbwt_rle *bwt, const uint64_t *rows, size_t n, uint64_t max_steps, uint8_t *out_symbols, uint64_t *out_steps, uint8_t *out_stops,
                        uint64_t *out_last, uint64_t *out_reads) {
    return walk_rows(bwt, rows, n, max_steps, true, out_symbols, out_steps, out_stops, out_last, out_reads, nullptr);
}

int msbwt_rle_walk_rows_device(const msbwt_rle *bwt, const void *d_rows, size_t n, uint64_t max_steps, void *d_out_symbols, void *d_out_steps, void *d_out_stops,
                               void *d_out_last, void *d_out_reads, void *hip_stream) {
    return walk_rows(bwt, d_rows, n, max_steps, false, d_out_symbols, d_out_steps, d_out_stops, d_out_last, d_out_reads, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_extract_reads(const msbwt_rle *bwt, const uint64_t *read_ids, uint64_t first_read, size_t n, uint64_t max_len, uint8_t *out_symbols, uint64_t *out_offsets,
                            uint64_t capacity_symbols, uint64_t *out_symbol_total, uint64_t *out_truncated) {
    return extract_reads(bwt, read_ids, first_read, n, max_len, true, out_symbols, out_offsets, capacity_symbols, out_symbol_total, out_truncated, nullptr);
}

int msbwt_rle_extract_reads_device(const msbwt_rle *bwt, const void *d_read_ids, uint64_t first_read, size_t n, uint64_t max_len, void *d_out_symbols, void *d_out_offsets,
                                   uint64_t capacity_symbols, uint64_t *out_symbol_total, uint64_t *out_truncated, void *hip_stream) {
    return extract_reads(bwt, d_read_ids, first_read, n, max_len, false, d_out_symbols, d_out_offsets, capacity_symbols, out_symbol_total, out_truncated,
                         static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_walk_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::walk_info, out); }

int msbwt_rle_set_walk_piece(msbwt_rle *bwt, uint64_t walks) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    if (walks > kWalkMaxPiece) {
        std::lock_guard<std::mutex> lock(bwt->mu);
        return fail(bwt, MSBWT_ERR_INVALID_ARG, "a piece of left walks is at most 2^28 walks (0 = automatic)");
    }
    return set_locked(bwt, bwt->walk_piece, walks);
}

int msbwt_walk_plan(uint64_t n, uint64_t max_steps, int symbols, int host, uint64_t piece, uint64_t *device_bytes) {
    if (piece > kWalkMaxPiece) return MSBWT_ERR_INVALID_ARG;
    if (walk_too_large(n, max_steps)) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) *device_bytes = n ? walk_layout(walk_piece_walks(n, piece), max_steps, symbols != 0, host != 0).bytes : 0;
    return MSBWT_OK;
}

}  // extern "C"
