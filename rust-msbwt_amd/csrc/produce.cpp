// The producers: the BWT built from reads and the merges, handed to the caller or loaded in place.
// Calls reads_build.hip and merge*.hip through their headers, and the loader through install and release_index only.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "handle.hpp"
#include "index_build.hpp"
#include "radix_sort.hpp"

namespace {

// The host-side checks of a read set (msbwt_rle_build_from_reads): nothing is launched before they pass.  *total = symbols of the
// text, every read's '$' included.
int check_reads(msbwt_rle *h, const uint8_t *reads, const uint64_t *read_offsets, size_t n_reads, int ascii, uint64_t *total) {
    *total = 0;
    if (n_reads == 0) return MSBWT_OK;
    if (!reads || !read_offsets) return fail(h, MSBWT_ERR_INVALID_ARG, "reads and read_offsets must not be null");
    for (size_t r = 0; r < n_reads; ++r)
        if (read_offsets[r + 1] < read_offsets[r]) return fail(h, MSBWT_ERR_INVALID_ARG, "read_offsets decrease at read " + std::to_string(r));
    const uint64_t lo = read_offsets[0], nbytes = read_offsets[n_reads] - lo;
    if (nbytes >= kMaxSymbols || nbytes + n_reads >= kMaxSymbols) return fail(h, MSBWT_ERR_TOO_LARGE, "the read set has 2^40 symbols or more");
    // ASCII: every byte but '$' has a code (string_util.rs:15-32); codes: 1..5.  Large sets are checked by a few threads.
    auto bad_in = [&](uint64_t from, uint64_t to) {
        unsigned bad = 0;
        if (ascii) for (uint64_t i = from; i < to; ++i) bad |= reads[lo + i] == '$';
        else for (uint64_t i = from; i < to; ++i) bad |= uint8_t(reads[lo + i] - 1u) > 4u;
        return bad != 0;
    };
    const unsigned workers = unsigned(std::min<uint64_t>(8, nbytes >> 24) + 1);
    std::atomic<bool> bad{false};
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < workers; ++t)
        pool.emplace_back([&, t] { if (bad_in(nbytes * t / workers, nbytes * (t + 1) / workers)) bad = true; });
    if (bad_in(0, nbytes / workers)) bad = true;
    for (auto &th : pool) th.join();
    if (bad) return fail(h, MSBWT_ERR_INVALID_SYMBOL, ascii ? "a read holds '$'" : "a read holds a symbol code outside 1..5");
    *total = nbytes + n_reads;
    return MSBWT_OK;
}

struct Produced {  // what a producer left in HBM: RLE bytes and, after a merge, the final state; freed at scope exit
    uint8_t *d_rle = nullptr, *d_state = nullptr;
    uint64_t rle_bytes = 0, state_bytes = 0;
    Produced() = default;
    Produced(const Produced &) = delete;
    Produced &operator=(const Produced &) = delete;
    ~Produced() {
        if (d_rle) (void)hipFree(d_rle);
        if (d_state) (void)hipFree(d_state);
    }
};

// The build itself, on the handle's device and stream: the RLE bytes stay in HBM.
int build_reads_on_device(msbwt_rle *h, const uint8_t *reads, const uint64_t *read_offsets, size_t n_reads, int ascii, uint64_t total, Produced *made) {
    if (int rc = ensure_runtime(h)) return rc;
    size_t free_bytes = 0, all_bytes = 0;
    HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
    const uint64_t piece = h->build_piece ? h->build_piece : plan_reads_build(total, free_bytes, 0).auto_piece;
    const char *wide = std::getenv("MSBWT_BUILD_WIDE");  // 64-bit positions below 2^32 symbols too (tests)
    ReadsBuildOutput out;
    const hipError_t e = build_rle_from_reads(reads, read_offsets, n_reads, ascii != 0, piece, wide && std::atoi(wide), h->stream, &out);
    made->d_rle = out.d_rle;
    made->rle_bytes = out.rle_bytes;
    std::copy(out.stage_ms, out.stage_ms + kReadsBuildStages, h->build_ms);
    h->build_pieces = out.pieces;
    if (std::getenv("MSBWT_VERBOSE"))
        std::fprintf(stderr, "[msbwt] build: %llu symbols, %llu pieces of at most %llu suffixes (limit %llu)\n", (unsigned long long)total,
                     (unsigned long long)out.pieces, (unsigned long long)out.largest_piece, (unsigned long long)piece);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, MSBWT_ERR_HIP, "build from reads: " + out.what + ": " + hipGetErrorString(e));
    }
    return MSBWT_OK;
}

// The host-side checks of a merge's inputs: nothing is launched before they pass.  Fills every span's `in`; *total = merged rows.
int check_merge_inputs(msbwt_rle *h, std::vector<MergeSpan> *spans, uint64_t *total) {
    *total = 0;
    for (size_t i = 0; i < spans->size(); ++i) {
        MergeSpan &span = (*spans)[i];
        switch (scan_merge_input(span.rle, span.len, &span.in)) {
            case MergeInputStatus::kOk: break;
            case MergeInputStatus::kInvalidSymbol: return fail(h, MSBWT_ERR_INVALID_SYMBOL, "input " + std::to_string(i) + " holds a symbol code >= 6");
            case MergeInputStatus::kTooLarge: return fail(h, MSBWT_ERR_TOO_LARGE, "input " + std::to_string(i) + " has 2^40 symbols or more");
        }
        *total += span.in.total;  // < 2^45
        if (*total >= kMaxSymbols) return fail(h, MSBWT_ERR_TOO_LARGE, "the merged BWT would have 2^40 symbols or more");
    }
    return MSBWT_OK;
}

// msbwt_rle_merge's two inputs as spans, checked
int check_merge_pair(msbwt_rle *h, const uint8_t *rle0, size_t len0, const uint8_t *rle1, size_t len1, std::vector<MergeSpan> *spans, uint64_t *total) {
    if ((!rle0 && len0) || (!rle1 && len1)) return fail(h, MSBWT_ERR_INVALID_ARG, "an input must not be null with a length");
    *spans = {MergeSpan{rle0, len0, MergeInput()}, MergeSpan{rle1, len1, MergeInput()}};
    return check_merge_inputs(h, spans, total);
}

// msbwt_rle_merge_many's packed inputs as spans, checked
int check_merge_packed(msbwt_rle *h, const uint8_t *rle, const uint64_t *offsets, size_t n, std::vector<MergeSpan> *spans, uint64_t *total) {
    *total = 0;
    if (n > MSBWT_MERGE_MAX_INPUTS) return fail(h, MSBWT_ERR_INVALID_ARG, std::to_string(n) + " inputs, one merge takes at most " + std::to_string(MSBWT_MERGE_MAX_INPUTS));
    if (n && !offsets) return fail(h, MSBWT_ERR_INVALID_ARG, "rle_offsets must not be null with inputs");
    for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(h, MSBWT_ERR_INVALID_ARG, "rle_offsets decrease at input " + std::to_string(i));
    if (n && !rle && offsets[n] > offsets[0]) return fail(h, MSBWT_ERR_INVALID_ARG, "rle must not be null with a length");
    spans->clear();
    for (size_t i = 0; i < n; ++i) {
        const size_t len = size_t(offsets[i + 1] - offsets[i]);
        spans->push_back(MergeSpan{len ? rle + offsets[i] : nullptr, len, MergeInput()});
    }
    return check_merge_inputs(h, spans, total);
}

void reset_merge_info(msbwt_rle *h) {
    std::fill(h->merge_ms, h->merge_ms + kMergeStages, 0.0);
    h->merge_iterations = 0;
}

// The merge itself (`run`: merge_rle_pair or merge_rle_many), on the handle's device and stream: the RLE bytes and the final state
// stay in HBM.
int merge_on_device(msbwt_rle *h, decltype(&merge_rle_many) run, const std::vector<MergeSpan> &spans, uint64_t total, Produced *made) {
    if (int rc = ensure_runtime(h)) return rc;
    MergeOutput out;
    const hipError_t e = run(spans.data(), spans.size(), h->stream, &out);
    made->d_rle = out.d_rle;
    made->rle_bytes = out.rle_bytes;
    made->d_state = out.d_state;
    made->state_bytes = out.state_bytes;
    std::copy(out.stage_ms, out.stage_ms + kMergeStages, h->merge_ms);
    h->merge_iterations = out.iterations;
    if (std::getenv("MSBWT_VERBOSE"))
        std::fprintf(stderr, "[msbwt] merge: %llu symbols in %zu inputs, %llu iterations\n", (unsigned long long)total, spans.size(), (unsigned long long)out.iterations);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, MSBWT_ERR_HIP, "merge: " + out.what + ": " + hipGetErrorString(e));
    }
    return MSBWT_OK;
}

// What the producers that hand their bytes to the caller share: `produce` leaves `noun`'s RLE bytes in HBM, they go to out_rle if
// its capacity allows (*out_len says what they take either way), the final state to out_state where the caller asked for it, and
// the copy's time to *copy_ms.
template <class Produce>
int produce_for_caller(msbwt_rle *h, Produce &&produce, const char *noun, uint8_t *out_rle, size_t cap, uint64_t *out_len, uint8_t *out_state, double *copy_ms) {
    DeviceScope scope(h->device);
    if (!scope.ok()) return fail(h, MSBWT_ERR_HIP, scope.why());
    Produced made;
    if (int rc = produce(&made)) return rc;
    *out_len = made.rle_bytes;
    if (made.rle_bytes > cap)
        return fail(h, MSBWT_ERR_INVALID_ARG, "out_rle holds " + std::to_string(cap) + " bytes, the " + noun + " takes " + std::to_string(made.rle_bytes));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(h, hipMemcpyAsync(out_rle, made.d_rle, made.rle_bytes, hipMemcpyDeviceToHost, h->stream));
    if (out_state) HIP_TRY(h, hipMemcpyAsync(out_state, made.d_state, size_t(made.state_bytes), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *copy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->err.clear();
    return MSBWT_OK;
}

// What the producers that load their result share: unless it is the empty BWT (`any`), the index gives way, `produce` leaves the
// RLE bytes in HBM, and they come down and are freed; then the loader of msbwt_rle_load_vector, on the same bytes.  With `sources`
// (msbwt_rle_load_merged_many_sources) the merge's final state, a byte per row, stays in HBM over the load and is attached from there.
template <class Produce>
int produce_and_install(msbwt_rle *h, bool any, Produce &&produce, size_t sources = 0) {
    DeviceScope scope(h->device);  // (install makes the same device current once more; `made` is freed inside this scope however the call ends)
    if (!scope.ok()) return fail(h, MSBWT_ERR_HIP, scope.why());
    std::vector<uint8_t> rle;
    Produced made;
    if (any) {
        release_index(h);  // its HBM is the producer's to use
        if (int rc = produce(&made)) return rc;
        rle.resize(size_t(made.rle_bytes));
        HIP_TRY(h, hipMemcpyAsync(rle.data(), made.d_rle, rle.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        (void)hipFree(made.d_rle);  // the loader's to use
        made.d_rle = nullptr;
        if (!sources && made.d_state) {
            (void)hipFree(made.d_state);
            made.d_state = nullptr;
        }
    }
    if (int rc = install(h, rle.data(), rle.size())) return rc;
    return sources ? attach_sources(h, nullptr, made.d_state, h->totals.total, sources) : int(MSBWT_OK);
}

}  // namespace

extern "C" {

int msbwt_rle_build_from_reads(msbwt_rle *h, const uint8_t *reads, const uint64_t *read_offsets, size_t n_reads, int ascii, uint8_t *out_rle, size_t cap,
                               uint64_t *out_len) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!out_len || (!out_rle && cap)) return fail(h, MSBWT_ERR_INVALID_ARG, "out_len must not be null, nor out_rle with a capacity");
    *out_len = 0;
    uint64_t total = 0;
    if (int rc = check_reads(h, reads, read_offsets, n_reads, ascii, &total)) return rc;
    std::fill(h->build_ms, h->build_ms + kReadsBuildStages, 0.0);
    h->build_pieces = 0;
    if (n_reads == 0) return MSBWT_OK;  // the empty BWT
    auto build = [&](Produced *made) { return build_reads_on_device(h, reads, read_offsets, n_reads, ascii, total, made); };
    return produce_for_caller(h, build, "BWT", out_rle, cap, out_len, nullptr, &h->build_ms[kStageCopyOut]);
}

int msbwt_rle_load_reads(msbwt_rle *h, const uint8_t *reads, const uint64_t *read_offsets, size_t n_reads, int ascii) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    uint64_t total = 0;
    if (int rc = check_reads(h, reads, read_offsets, n_reads, ascii, &total)) return rc;
    return produce_and_install(h, n_reads != 0, [&](Produced *made) { return build_reads_on_device(h, reads, read_offsets, n_reads, ascii, total, made); });
}

int msbwt_rle_merge(msbwt_rle *h, const uint8_t *rle0, size_t len0, const uint8_t *rle1, size_t len1, uint8_t *out_rle, size_t cap, uint64_t *out_len,
                    uint8_t *out_from_second) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!out_len || (!out_rle && cap)) return fail(h, MSBWT_ERR_INVALID_ARG, "out_len must not be null, nor out_rle with a capacity");
    *out_len = 0;
    std::vector<MergeSpan> spans;
    uint64_t total = 0;
    if (int rc = check_merge_pair(h, rle0, len0, rle1, len1, &spans, &total)) return rc;
    reset_merge_info(h);
    if (total == 0) return MSBWT_OK;  // the empty BWT
    auto merge = [&](Produced *made) { return merge_on_device(h, merge_rle_pair, spans, total, made); };
    return produce_for_caller(h, merge, "merged BWT", out_rle, cap, out_len, out_from_second, &h->merge_ms[kMergeCopyOut]);
}

int msbwt_rle_load_merged(msbwt_rle *h, const uint8_t *rle0, size_t len0, const uint8_t *rle1, size_t len1) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    std::vector<MergeSpan> spans;
    uint64_t total = 0;
    if (int rc = check_merge_pair(h, rle0, len0, rle1, len1, &spans, &total)) return rc;
    return produce_and_install(h, total != 0, [&](Produced *made) { return merge_on_device(h, merge_rle_pair, spans, total, made); });
}

int msbwt_rle_merge_many(msbwt_rle *h, const uint8_t *rle, const uint64_t *rle_offsets, size_t n_inputs, uint8_t *out_rle, size_t cap, uint64_t *out_len,
                         uint8_t *out_source) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!out_len || (!out_rle && cap)) return fail(h, MSBWT_ERR_INVALID_ARG, "out_len must not be null, nor out_rle with a capacity");
    *out_len = 0;
    std::vector<MergeSpan> spans;
    uint64_t total = 0;
    if (int rc = check_merge_packed(h, rle, rle_offsets, n_inputs, &spans, &total)) return rc;
    reset_merge_info(h);
    if (total == 0) return MSBWT_OK;  // the empty BWT
    auto merge = [&](Produced *made) { return merge_on_device(h, merge_rle_many, spans, total, made); };
    return produce_for_caller(h, merge, "merged BWT", out_rle, cap, out_len, out_source, &h->merge_ms[kMergeCopyOut]);
}

int msbwt_rle_load_merged_many(msbwt_rle *h, const uint8_t *rle, const uint64_t *rle_offsets, size_t n_inputs) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    std::vector<MergeSpan> spans;
    uint64_t total = 0;
    if (int rc = check_merge_packed(h, rle, rle_offsets, n_inputs, &spans, &total)) return rc;
    return produce_and_install(h, total != 0, [&](Produced *made) { return merge_on_device(h, merge_rle_many, spans, total, made); });
}

int msbwt_rle_load_merged_many_sources(msbwt_rle *h, const uint8_t *rle, const uint64_t *rle_offsets, size_t n_inputs) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    std::vector<MergeSpan> spans;
    uint64_t total = 0;
    if (int rc = check_merge_packed(h, rle, rle_offsets, n_inputs, &spans, &total)) return rc;
    return produce_and_install(h, total != 0, [&](Produced *made) { return merge_on_device(h, merge_rle_many, spans, total, made); }, n_inputs);
}

int msbwt_merge_many_plan(const uint64_t *totals, size_t n_inputs, uint64_t *device_bytes) {
    if (n_inputs > MSBWT_MERGE_MAX_INPUTS || (!totals && n_inputs)) return MSBWT_ERR_INVALID_ARG;
    uint64_t total = 0;
    for (size_t i = 0; i < n_inputs; ++i) {
        if (totals[i] >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
        total += totals[i];  // < 2^45
    }
    if (total >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) *device_bytes = plan_merge_many(total);
    return MSBWT_OK;
}

int msbwt_merge_plan(uint64_t total0, uint64_t total1, uint64_t *device_bytes) {
    if (total0 >= kMaxSymbols || total1 >= kMaxSymbols || total0 + total1 >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) *device_bytes = plan_merge(total0, total1);
    return MSBWT_OK;
}

size_t msbwt_merge_tile(void) { return kMergeTile; }

int msbwt_rle_merge_info(const msbwt_rle *ch, uint64_t *iterations, double *out_ms) {
    Call c(ch);
    if (!c.h) return MSBWT_ERR_INVALID_ARG;
    if (iterations) *iterations = c.h->merge_iterations;
    if (out_ms) std::copy(c.h->merge_ms, c.h->merge_ms + kMergeStages, out_ms);
    return MSBWT_OK;
}

int msbwt_rle_set_build_piece(msbwt_rle *h, uint64_t suffixes) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    return set_locked(h, h->build_piece, suffixes);
}

int msbwt_build_reads_plan(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t piece, uint64_t *auto_piece, uint64_t *device_bytes) {
    if (total_symbols >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    const ReadsBuildPlan p = plan_reads_build(total_symbols, free_hbm_bytes, piece);
    if (auto_piece) *auto_piece = p.auto_piece;
    if (device_bytes) *device_bytes = p.device_bytes;
    return MSBWT_OK;
}

size_t msbwt_build_reads_sort_tile(void) { return kRadixSortTile; }

int msbwt_rle_build_stage_ms(const msbwt_rle *ch, double *out_ms, uint64_t *out_pieces) {
    Call c(ch);
    if (!c.h || !out_ms) return MSBWT_ERR_INVALID_ARG;
    std::copy(c.h->build_ms, c.h->build_ms + kReadsBuildStages, out_ms);
    if (out_pieces) *out_pieces = c.h->build_pieces;
    return MSBWT_OK;
}

}  // extern "C"
