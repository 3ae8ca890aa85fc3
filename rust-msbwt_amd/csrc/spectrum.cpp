// The k-mers of a loaded index: abundance spectrum and k-mer dump (msbwt_rle_kmer_spectrum, msbwt_rle_enumerate_kmers[_device]), their
// knobs, and the same two with a k-mer and its reverse complement merged into one class (msbwt_rle_canonical_kmer_spectrum,
// msbwt_rle_enumerate_canonical_kmers[_device]: canonical.hpp; the other strand is counted by query.cpp's packed search).  Calls
// spectrum.hip and canonical.hip through their headers and handle.hpp.  The k-mers by source (msbwt_rle_kmer_spectrum_by_source,
// msbwt_rle_enumerate_kmers_by_source[_device]: source_spectrum.hpp) are the same staged walk with the source sink behind it, and the
// k-mer graph (msbwt_rle_enumerate_kmer_graph[_device], msbwt_rle_kmer_graph_degrees: kmer_graph.hpp) is the sorted dump's counting
// walk followed by the staged walk with the edge pass behind it.  All scratch is allocated per call and freed before the call returns.
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "canonical.hpp"
#include "handle.hpp"
#include "kmer_graph.hpp"
#include "run_encode.hpp"
#include "source_spectrum.hpp"
#include "spectrum.hpp"

namespace {

static_assert(MSBWT_SPECTRUM_MIN_FRONTIER == kSpectrumMinFrontier && MSBWT_SPECTRUM_INFO_WORDS == 4 + kSpectrumMaxK + 1 + 3, "the header's constants");
constexpr uint64_t kRecordBytes = 3 * sizeof(uint64_t);  // k-mer, count, l

// bytes of scratch a call allocates; MSBWT_ERR_TOO_LARGE for what no index can be
int plan_bytes(uint64_t total_rows, uint64_t free_bytes, uint64_t frontier, uint64_t records, bool sorted, uint64_t *bytes) {
    if (total_rows >= kMaxSymbols || records >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    *bytes = spectrum_work_bytes(spectrum_frontier_nodes(total_rows, free_bytes, frontier)) + (sorted ? spectrum_rank_bytes(total_rows) : 0) + records * kRecordBytes;
    return MSBWT_OK;
}

// where the walk starts: the flat direct table when it is shallower than k, else the root
SpectrumSeeds seeds_of(const msbwt_rle *h, size_t k) {
    const DirectTable &t = h->table;
    if (t.entries && !t.packed && t.depth > 0 && size_t(t.depth) < k) return SpectrumSeeds{t.entries, t.depth};
    return SpectrumSeeds{};
}

struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    uint64_t us() const { return uint64_t(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count()); }
};

void record(msbwt_rle *h, const SpectrumInfo &info, const Clock &clock, uint64_t scratch_bytes = 0) {
    h->spectrum_scratch = scratch_bytes;
    uint64_t *w = h->spectrum_info;
    std::fill(w, w + MSBWT_SPECTRUM_INFO_WORDS, 0ull);
    w[0] = info.k;
    w[1] = info.seed_depth;
    w[2] = info.chunks;
    w[3] = info.retries;
    std::copy(info.nodes, info.nodes + kSpectrumMaxK + 1, w + 4);
    const uint64_t us = clock.us();
    w[37] = (us + 500) / 1000;
    w[38] = us;
    w[39] = info.descents;
}

// the scratch of one call: freed when it goes out of scope
struct Scratch {
    Arena arena;
    void *work = nullptr, *rank = nullptr;
    uint64_t frontier = 0;
    uint64_t *rc_words = nullptr, *rc_counts = nullptr;  // canonical calls: the other strand of a chunk's k-mers, `frontier` words each
    unsigned long long *totals = nullptr;                // and the words of CanonicalSink::totals
};

// work (and, wanted, the rank scratch or the canonical calls' staging) in HBM, or MSBWT_ERR_HIP naming the bytes
int take_scratch(msbwt_rle *h, Scratch &s, bool rank, uint64_t extra_bytes, const char *what, bool canonical = false) {
    size_t free_bytes = 0, all_bytes = 0;
    HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
    const uint64_t total = h->totals.total;
    s.frontier = spectrum_frontier_nodes(total, free_bytes, h->spectrum_frontier);
    const uint64_t work_bytes = spectrum_work_bytes(s.frontier), rank_bytes = rank ? spectrum_rank_bytes(total) : 0;
    if (canonical) extra_bytes += s.frontier * kCanonicalStageBytes;
    const std::string need = std::string(what) + ": " + std::to_string(work_bytes + rank_bytes + extra_bytes) + " bytes of HBM needed while it runs";
    if (free_bytes < work_bytes + rank_bytes + extra_bytes) return fail(h, MSBWT_ERR_HIP, need);
    if (s.arena.take(&s.work, work_bytes) != hipSuccess || (rank && s.arena.take(&s.rank, rank_bytes) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(h, MSBWT_ERR_HIP, need);
    }
    if (canonical && (s.arena.take(&s.rc_words, s.frontier * 8) != hipSuccess || s.arena.take(&s.rc_counts, s.frontier * 8) != hipSuccess ||
                      s.arena.take(&s.totals, kCanonicalTotalWords * 8) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(h, MSBWT_ERR_HIP, need);
    }
    return MSBWT_OK;
}

// Both forms of the dump.  host: the out_* are host arrays, filled through a device staging of n records; else device arrays.
int enumerate(const msbwt_rle *ch, size_t k, uint64_t min_count, uint64_t max_count, int sorted, bool host, void *out_kmers, void *out_counts, void *out_l,
              uint64_t capacity, uint64_t *out_n, hipStream_t stream, int which) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_kmers needs 1 <= k <= 32");
    if (max_count != 0 && min_count > max_count) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_kmers: min_count > max_count");
    if (!out_n || (capacity && !out_kmers)) return fail(h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    if (host) stream = h->stream;
    const Clock clock;
    *out_n = 0;
    SpectrumInfo info;
    info.k = k;
    if (h->totals.total == 0) {
        record(h, info, clock);
        return MSBWT_OK;
    }
    const bool rank = sorted != 0 && capacity != 0;
    Scratch s;
    if (int rc = take_scratch(h, s, rank, 0, "enumerate_kmers")) return rc;
    const IndexView v = view_of(h);
    const SpectrumSeeds seeds = seeds_of(h, k);
    uint64_t n = 0;
    HIP_TRY(h, spectrum_count(v, seeds, uint32_t(k), min_count, max_count, s.work, s.frontier, s.rank, &n, &info, stream));
    *out_n = n;
    record(h, info, clock, s.arena.taken);
    if (capacity == 0 || n == 0) return MSBWT_OK;
    if (capacity < n)
        return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_kmers: capacity " + std::to_string(capacity) + " is less than the n = " + std::to_string(n) + " k-mers that qualify");
    uint64_t *d_kmers = static_cast<uint64_t *>(out_kmers), *d_counts = static_cast<uint64_t *>(out_counts), *d_l = static_cast<uint64_t *>(out_l);
    uint64_t *stage = nullptr;
    if (host) {  // records staged in HBM, then copied out
        const uint64_t columns = 1 + (out_counts ? 1 : 0) + (out_l ? 1 : 0);
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
        if (free_bytes < n * columns * 8 || s.arena.take(&stage, n * columns * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, "enumerate_kmers: " + std::to_string(n * columns * 8) + " more bytes of HBM needed for the records");
        }
        d_kmers = stage;
        d_counts = out_counts ? stage + n : nullptr;
        d_l = out_l ? stage + n * (out_counts ? 2 : 1) : nullptr;
        capacity = n;
    }
    HIP_TRY(h, spectrum_dump(v, seeds, uint32_t(k), min_count, max_count, s.work, s.frontier, s.rank, d_kmers, d_counts, d_l, capacity, h->d_flags + which, &info,
                             stream));
    record(h, info, clock, s.arena.taken);
    if (!host) return MSBWT_OK;  // (a fault is in the device status word: msbwt_rle_device_status)
    HIP_TRY(h, hipMemcpyAsync(out_kmers, d_kmers, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_counts) HIP_TRY(h, hipMemcpyAsync(out_counts, d_counts, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_l) HIP_TRY(h, hipMemcpyAsync(out_l, d_l, n * 8, hipMemcpyDeviceToHost, stream));
    return status_of(h, stream, which);  // synchronises
}

// ---- canonical k-mers ----

// One walk of a canonical call: chunk by chunk the k-mers at least `prune` wide are staged, their reverse complements written as packed
// words and counted by the packed search, and the classes they emit go to `sink` (its totals: s.totals, copied to totals[] at the end).
// Synchronises the stream.
int canonical_walk(msbwt_rle *h, const Scratch &s, size_t k, uint64_t prune, CanonicalSink sink, SpectrumInfo *info, hipStream_t stream, int which, uint64_t *totals) {
    sink.totals = s.totals;
    HIP_TRY(h, hipMemsetAsync(s.totals, 0, kCanonicalTotalWords * 8, stream));
    int search_rc = MSBWT_OK;
    const SpectrumChunkHook per_chunk = [&](const void *d_kmers, uint64_t m) {
        const hipError_t e = launch_canonical_rc(d_kmers, m, uint32_t(k), s.rc_words, stream);
        if (e != hipSuccess) return e;
        if ((search_rc = launch_count_2bit(h, s.rc_words, k, size_t(m), s.rc_counts, stream, which)) != MSBWT_OK) return hipErrorUnknown;
        return launch_canonical_combine(d_kmers, s.rc_words, s.rc_counts, m, sink, stream);
    };
    const hipError_t walked = spectrum_stage(view_of(h), seeds_of(h, k), uint32_t(k), prune, s.work, s.frontier, per_chunk, info, stream);
    if (search_rc) return search_rc;
    HIP_TRY(h, walked);
    HIP_TRY(h, hipMemcpyAsync(totals, s.totals, kCanonicalTotalWords * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return MSBWT_OK;
}

// Both forms of the canonical dump, as enumerate() above: records (canonical word, own, other), in the order the walk produces them.
int enumerate_canonical(const msbwt_rle *ch, size_t k, uint64_t min_count, uint64_t max_count, bool host, void *out_kmers, void *out_own, void *out_other,
                        uint64_t capacity, uint64_t *out_n, hipStream_t stream, int which) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_canonical_kmers needs 1 <= k <= 32");
    if (max_count != 0 && min_count > max_count) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_canonical_kmers: min_count > max_count");
    if (!out_n || (capacity && !out_kmers)) return fail(h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    if (host) stream = h->stream;
    const Clock clock;
    *out_n = 0;
    SpectrumInfo info;
    info.k = k;
    if (h->totals.total == 0) {
        record(h, info, clock);
        return MSBWT_OK;
    }
    Scratch s;
    if (int rc = take_scratch(h, s, false, 0, "enumerate_canonical_kmers", true)) return rc;
    CanonicalSink sink{};
    sink.mode = kCanonicalCount;
    sink.min = std::max<uint64_t>(min_count, 1);
    sink.max = max_count ? max_count : ~0ull;
    // of two strands whose counts sum to sink.min or more, the one that emits the class -- the larger -- has at least half of it
    const uint64_t prune = sink.min / 2 + sink.min % 2;
    uint64_t totals[kCanonicalTotalWords] = {};
    if (int rc = canonical_walk(h, s, k, prune, sink, &info, stream, which, totals)) return rc;
    const uint64_t n = totals[kCanonicalClasses];
    *out_n = n;
    record(h, info, clock, s.arena.taken);
    if (capacity == 0 || n == 0) return host ? status_of(h, stream, which) : int(MSBWT_OK);
    if (capacity < n)
        return fail(h, MSBWT_ERR_INVALID_ARG,
                    "enumerate_canonical_kmers: capacity " + std::to_string(capacity) + " is less than the n = " + std::to_string(n) + " classes that qualify");
    sink.mode = kCanonicalAppend;
    sink.kmers = static_cast<uint64_t *>(out_kmers);
    sink.own = static_cast<uint64_t *>(out_own);
    sink.other = static_cast<uint64_t *>(out_other);
    sink.capacity = capacity;
    sink.flags = h->d_flags + which;
    if (host) {  // records staged in HBM, then copied out
        const uint64_t columns = 1 + (out_own ? 1 : 0) + (out_other ? 1 : 0);
        uint64_t *stage = nullptr;
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
        if (free_bytes < n * columns * 8 || s.arena.take(&stage, n * columns * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, "enumerate_canonical_kmers: " + std::to_string(n * columns * 8) + " more bytes of HBM needed for the records");
        }
        sink.kmers = stage;
        sink.own = out_own ? stage + n : nullptr;
        sink.other = out_other ? stage + n * (out_own ? 2 : 1) : nullptr;
        sink.capacity = n;
    }
    if (int rc = canonical_walk(h, s, k, prune, sink, &info, stream, which, totals)) return rc;
    record(h, info, clock, s.arena.taken);
    if (!host) return MSBWT_OK;  // (a fault is in the device status word: msbwt_rle_device_status)
    HIP_TRY(h, hipMemcpyAsync(out_kmers, sink.kmers, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_own) HIP_TRY(h, hipMemcpyAsync(out_own, sink.own, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_other) HIP_TRY(h, hipMemcpyAsync(out_other, sink.other, n * 8, hipMemcpyDeviceToHost, stream));
    return status_of(h, stream, which);  // synchronises
}

// ---- k-mers by source ----

int need_sources(msbwt_rle *h) { return h->sources.n_sources ? int(MSBWT_OK) : fail(h, MSBWT_ERR_NOT_LOADED, "no sources attached"); }

// bytes of scratch a by-source call allocates: the walk's (plan_bytes), the sink's fixed words, and per record staged for a host dump
// the word, l and the S counts.  Nothing here grows with frontier x sources.
int by_source_plan_bytes(uint64_t total_rows, uint64_t free_bytes, uint64_t frontier, size_t n_sources, uint64_t records, bool sorted, uint64_t *bytes) {
    if (n_sources < 1 || n_sources > kSourceMax) return MSBWT_ERR_INVALID_ARG;
    if (records >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    if (int rc = plan_bytes(total_rows, free_bytes, frontier, 0, sorted, bytes)) return rc;
    *bytes += kSourceSinkFixedBytes + records * (2 + n_sources) * sizeof(uint64_t);
    return MSBWT_OK;
}

// the sink's fixed words: the limits, then the totals
struct SourceFixed {
    uint64_t *limits = nullptr;
    unsigned long long *totals = nullptr;
};

int take_source_fixed(msbwt_rle *h, Scratch &s, SourceFixed &f, const char *what) {
    if (s.arena.take(&f.limits, kSourceSinkFixedBytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, MSBWT_ERR_HIP, std::string(what) + ": " + std::to_string(kSourceSinkFixedBytes) + " more bytes of HBM needed for the sink");
    }
    f.totals = reinterpret_cast<unsigned long long *>(f.limits + 2 * kSourceMax);
    return MSBWT_OK;
}

// One walk of a by-source call: chunk by chunk the k-mers at least `prune` wide are staged and handed to the source sink (its totals:
// f.totals, copied to totals[] at the end).  Synchronises the stream.
int by_source_walk(msbwt_rle *h, const Scratch &s, const SourceFixed &f, size_t k, uint64_t prune, SourceSink sink, SpectrumInfo *info, hipStream_t stream, uint64_t *totals) {
    sink.totals = f.totals;
    sink.limits = f.limits;
    HIP_TRY(h, hipMemsetAsync(f.totals, 0, kSourceTotalWords * 8, stream));
    const SourceView view = h->sources.view(h->totals.total);
    const SpectrumChunkHook per_chunk = [&](const void *d_kmers, uint64_t m) { return launch_source_sink(d_kmers, m, view, sink, stream); };
    HIP_TRY(h, spectrum_stage(view_of(h), seeds_of(h, k), uint32_t(k), prune, s.work, s.frontier, per_chunk, info, stream));
    HIP_TRY(h, hipMemcpyAsync(totals, f.totals, kSourceTotalWords * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return MSBWT_OK;
}

uint64_t add_saturating(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// Both forms of the by-source dump, as enumerate() above: records (word, c_0 .. c_{S-1}, l).
int enumerate_by_source(const msbwt_rle *ch, size_t k, const uint64_t *min_counts, const uint64_t *max_counts, uint64_t min_total, uint64_t max_total, int sorted, bool host,
                        void *out_kmers, void *out_counts, void *out_l, uint64_t capacity, uint64_t *out_n, hipStream_t stream, int which) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (int rc = need_sources(h)) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_kmers_by_source needs 1 <= k <= 32");
    const uint64_t S = h->sources.n_sources;
    uint64_t limits[2 * kSourceMax];
    uint64_t prune = std::max<uint64_t>(min_total, 1), min_sum = 0;
    for (uint32_t s = 0; s < kSourceMax; ++s) {
        limits[s] = s < S && min_counts ? min_counts[s] : 0ull;
        limits[kSourceMax + s] = s < S && max_counts ? max_counts[s] : ~0ull;
        if (limits[s] > limits[kSourceMax + s]) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_kmers_by_source: min_counts[" + std::to_string(s) + "] > max_counts[" + std::to_string(s) + "]");
        min_sum = add_saturating(min_sum, limits[s]);
    }
    if (max_total != 0 && min_total > max_total) return fail(h, MSBWT_ERR_INVALID_ARG, "enumerate_kmers_by_source: min_total > max_total");
    if (!out_n || (capacity && !out_kmers)) return fail(h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    if (host) stream = h->stream;
    const Clock clock;
    *out_n = 0;
    SpectrumInfo info;
    info.k = k;
    if (h->totals.total == 0) {
        record(h, info, clock);
        return MSBWT_OK;
    }
    // a suffix's total is at least the k-mer's, and the k-mer's is at least the sum of its minima
    prune = std::max(prune, min_sum);
    const bool rank = sorted != 0 && capacity != 0;
    Scratch s;
    if (int rc = take_scratch(h, s, rank, kSourceSinkFixedBytes, "enumerate_kmers_by_source")) return rc;
    SourceFixed f;
    if (int rc = take_source_fixed(h, s, f, "enumerate_kmers_by_source")) return rc;
    HIP_TRY(h, hipMemcpyAsync(f.limits, limits, sizeof limits, hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));  // (the limits are this frame's)
    SourceSink sink{};
    sink.mode = kSourceSinkCount;
    sink.min_total = std::max<uint64_t>(min_total, 1);
    sink.max_total = max_total ? max_total : ~0ull;
    sink.flags = h->d_flags + which;
    SpectrumRank r{};
    if (rank) {
        r = spectrum_rank_view(s.rank, h->totals.total);
        HIP_TRY(h, spectrum_rank_clear(r, stream));
        sink.bitmap = r.bitmap;
    }
    uint64_t totals[kSourceTotalWords] = {};
    if (int rc = by_source_walk(h, s, f, k, prune, sink, &info, stream, totals)) return rc;
    const uint64_t n = totals[kSourcePassed];
    *out_n = n;
    record(h, info, clock, s.arena.taken);
    if (capacity == 0 || n == 0) return host ? status_of(h, stream, which) : int(MSBWT_OK);
    if (capacity < n)
        return fail(h, MSBWT_ERR_INVALID_ARG,
                    "enumerate_kmers_by_source: capacity " + std::to_string(capacity) + " is less than the n = " + std::to_string(n) + " k-mers that qualify");
    sink.mode = rank ? kSourceSinkScatter : kSourceSinkAppend;
    sink.kmers = static_cast<uint64_t *>(out_kmers);
    sink.counts = static_cast<uint64_t *>(out_counts);
    sink.l = static_cast<uint64_t *>(out_l);
    sink.capacity = capacity;
    if (rank) {
        HIP_TRY(h, spectrum_rank_close(r, stream));
        sink.prefix = r.prefix;
    }
    if (host) {  // records staged in HBM, then copied out
        const uint64_t words = n * (1 + (out_counts ? S : 0) + (out_l ? 1 : 0));
        uint64_t *stage = nullptr;
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
        if (free_bytes < words * 8 || s.arena.take(&stage, words * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, "enumerate_kmers_by_source: " + std::to_string(words * 8) + " more bytes of HBM needed for the records");
        }
        sink.kmers = stage;
        sink.l = out_l ? stage + n : nullptr;
        sink.counts = out_counts ? stage + n * (out_l ? 2 : 1) : nullptr;
        sink.capacity = n;
    }
    if (int rc = by_source_walk(h, s, f, k, prune, sink, &info, stream, totals)) return rc;
    record(h, info, clock, s.arena.taken);
    if (!host) return MSBWT_OK;  // (a fault is in the device status word: msbwt_rle_device_status)
    HIP_TRY(h, hipMemcpyAsync(out_kmers, sink.kmers, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_counts) HIP_TRY(h, hipMemcpyAsync(out_counts, sink.counts, n * S * 8, hipMemcpyDeviceToHost, stream));
    if (out_l) HIP_TRY(h, hipMemcpyAsync(out_l, sink.l, n * 8, hipMemcpyDeviceToHost, stream));
    return status_of(h, stream, which);  // synchronises
}

// ---- the k-mer graph ----

// bytes of scratch a graph call that fills buffers (or the degree table) allocates: the sorted walk's (plan_bytes), the degree counters,
// the edge bytes of `records` nodes as whole 32-bit words, and `columns` 8-byte words per record staged for a host dump
int graph_plan_bytes(uint64_t total_rows, uint64_t free_bytes, uint64_t records, uint64_t columns, uint64_t *bytes) {
    if (records >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    if (int rc = plan_bytes(total_rows, free_bytes, 0, 0, true, bytes)) return rc;
    *bytes += kGraphFixedBytes + graph_edge_words(records) * 4 + records * columns * 8;
    return MSBWT_OK;
}

// The dump (both forms) and the degree table (table != nullptr: no record outputs, *out_n = the nodes, *out_edge_count = the edges).
// host: the out_* are host arrays, filled through a device staging of n records; else device arrays.
int kmer_graph(const msbwt_rle *ch, size_t k, uint64_t min_count, uint64_t min_edge, bool host, void *out_kmers, void *out_counts, void *out_l, void *out_edges,
               uint64_t capacity, uint64_t *out_n, uint64_t *table, uint64_t *out_edge_count, hipStream_t stream, int which) {
    const bool degrees = table != nullptr;
    const char *what = degrees ? "kmer_graph_degrees" : "enumerate_kmer_graph";
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, std::string(what) + " needs 1 <= k <= 32");
    const uint64_t m = std::max<uint64_t>(min_count, 1), me = min_edge ? min_edge : m;
    if (me < m) return fail(h, MSBWT_ERR_INVALID_ARG, std::string(what) + ": min_edge is below the node threshold (0 = the node threshold)");
    if (!degrees && !out_n) return fail(h, MSBWT_ERR_INVALID_ARG, "null pointer");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    if (host) stream = h->stream;
    const Clock clock;
    uint64_t n = 0;
    if (out_n) *out_n = 0;
    if (out_edge_count) *out_edge_count = 0;
    if (degrees) std::fill(table, table + kGraphTableWords, 0ull);
    SpectrumInfo info;
    info.k = k;
    if (h->totals.total == 0) {
        record(h, info, clock);
        return MSBWT_OK;
    }
    const bool fill = degrees || capacity != 0;
    Scratch s;
    if (int rc = take_scratch(h, s, fill, fill ? kGraphFixedBytes : 0, what)) return rc;
    const IndexView v = view_of(h);
    const SpectrumSeeds seeds = seeds_of(h, k);
    HIP_TRY(h, spectrum_count(v, seeds, uint32_t(k), m, 0, s.work, s.frontier, s.rank, &n, &info, stream));
    if (out_n) *out_n = n;
    record(h, info, clock, s.arena.taken);
    if (!fill || n == 0) return MSBWT_OK;
    if (!degrees && capacity < n)
        return fail(h, MSBWT_ERR_INVALID_ARG, std::string(what) + ": capacity " + std::to_string(capacity) + " is less than the n = " + std::to_string(n) + " k-mers that qualify");
    // one allocation: the records staged for a host dump | the degree counters | the edge words
    const uint64_t columns = host && !degrees ? (out_kmers ? 1 : 0) + (out_counts ? 1 : 0) + (out_l ? 1 : 0) : 0;
    const uint64_t stage_bytes = n * columns * 8, edge_bytes = graph_edge_words(n) * 4, more = stage_bytes + kGraphFixedBytes + edge_bytes;
    char *block = nullptr;
    size_t free_bytes = 0, all_bytes = 0;
    HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
    if (free_bytes < more || s.arena.take(&block, more) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, MSBWT_ERR_HIP, std::string(what) + ": " + std::to_string(more) + " more bytes of HBM needed for the edge bytes and the records");
    }
    uint64_t *stage = reinterpret_cast<uint64_t *>(block), *d_table = reinterpret_cast<uint64_t *>(block + stage_bytes);
    uint32_t *edge_words = reinterpret_cast<uint32_t *>(block + stage_bytes + kGraphFixedBytes);
    HIP_TRY(h, hipMemsetAsync(d_table, 0, kGraphFixedBytes + edge_bytes, stream));
    const SpectrumRank r = spectrum_rank_view(s.rank, h->totals.total);
    GraphSink sink{};
    sink.bitmap = r.bitmap;
    sink.prefix = r.prefix;
    sink.edge_words = edge_words;
    sink.n = n;
    sink.min_edge = me;
    sink.flags = h->d_flags + which;
    if (host && !degrees) {
        uint64_t *next = stage;
        auto column = [&](const void *wanted) {
            uint64_t *at = wanted ? next : nullptr;
            if (wanted) next += n;
            return at;
        };
        sink.kmers = column(out_kmers);
        sink.counts = column(out_counts);
        sink.l = column(out_l);
    } else if (!degrees) {
        sink.kmers = static_cast<uint64_t *>(out_kmers);
        sink.counts = static_cast<uint64_t *>(out_counts);
        sink.l = static_cast<uint64_t *>(out_l);
    }
    const SpectrumChunkHook per_chunk = [&](const void *d_nodes, uint64_t nodes) { return launch_graph_edges(v, d_nodes, nodes, sink, stream); };
    HIP_TRY(h, spectrum_stage(v, seeds, uint32_t(k), m, s.work, s.frontier, per_chunk, &info, stream));
    record(h, info, clock, s.arena.taken);
    if (degrees) {
        HIP_TRY(h, launch_graph_degrees(edge_words, n, d_table, stream));
        HIP_TRY(h, hipMemcpyAsync(table, d_table, kGraphTableWords * 8, hipMemcpyDeviceToHost, stream));
        if (int rc = status_of(h, stream, which)) return rc;  // synchronises
        uint64_t edges = 0;
        for (uint32_t i = 0; i < kGraphTableWords; ++i) edges += uint64_t(i / kGraphDegrees) * table[i];  // (the in-degrees; the out-degrees sum to the same)
        if (out_edge_count) *out_edge_count = edges;
        return MSBWT_OK;
    }
    if (!host) {  // (a fault is in the device status word: msbwt_rle_device_status)
        if (out_edges) HIP_TRY(h, hipMemcpyAsync(out_edges, edge_words, n, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));  // (the last chunk's edge pass, and the scratch is freed on return)
        return MSBWT_OK;
    }
    if (out_kmers) HIP_TRY(h, hipMemcpyAsync(out_kmers, sink.kmers, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_counts) HIP_TRY(h, hipMemcpyAsync(out_counts, sink.counts, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_l) HIP_TRY(h, hipMemcpyAsync(out_l, sink.l, n * 8, hipMemcpyDeviceToHost, stream));
    if (out_edges) HIP_TRY(h, hipMemcpyAsync(out_edges, edge_words, n, hipMemcpyDeviceToHost, stream));
    return status_of(h, stream, which);  // synchronises
}

}  // namespace

extern "C" {

int msbwt_rle_kmer_spectrum(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_distinct, uint64_t *out_occurrences) {
    Call c(bwt);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, "kmer_spectrum needs 1 <= k <= 32");
    if (n_bins < 2 || !out_hist) return fail(h, MSBWT_ERR_INVALID_ARG, "kmer_spectrum needs a histogram of at least 2 bins");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    const Clock clock;
    uint64_t scratch_bytes = 0;
    SpectrumInfo info;
    info.k = k;
    uint64_t distinct = 0, occurrences = 0;
    std::fill(out_hist, out_hist + n_bins, 0ull);
    if (h->totals.total != 0) {
        Scratch s;
        if (int rc = take_scratch(h, s, false, uint64_t(n_bins) * 8, "kmer_spectrum")) return rc;
        uint64_t *d_hist = nullptr;
        if (s.arena.take(&d_hist, uint64_t(n_bins) * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, "kmer_spectrum: " + std::to_string(uint64_t(n_bins) * 8) + " bytes of HBM needed for the histogram");
        }
        HIP_TRY(h, hipMemsetAsync(d_hist, 0, uint64_t(n_bins) * 8, h->stream));
        HIP_TRY(h, spectrum_histogram(view_of(h), seeds_of(h, k), uint32_t(k), s.work, s.frontier, d_hist, n_bins, &distinct, &occurrences, &info, h->stream));
        HIP_TRY(h, hipMemcpyAsync(out_hist, d_hist, uint64_t(n_bins) * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        scratch_bytes = s.arena.taken;
    }
    if (out_distinct) *out_distinct = distinct;
    if (out_occurrences) *out_occurrences = occurrences;
    record(h, info, clock, scratch_bytes);
    return MSBWT_OK;
}

int msbwt_rle_enumerate_kmers(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted, uint64_t *out_kmers2bit, uint64_t *out_counts,
                              uint64_t *out_l, uint64_t capacity, uint64_t *out_n) {
    return enumerate(bwt, k, min_count, max_count, sorted, true, out_kmers2bit, out_counts, out_l, capacity, out_n, nullptr, kHostFlags);
}

int msbwt_rle_enumerate_kmers_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted, void *d_out_kmers2bit, void *d_out_counts,
                                     void *d_out_l, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return enumerate(bwt, k, min_count, max_count, sorted, false, d_out_kmers2bit, d_out_counts, d_out_l, capacity, out_n, static_cast<hipStream_t>(hip_stream),
                     kDeviceFlags);
}

int msbwt_rle_set_spectrum_frontier(msbwt_rle *bwt, uint64_t nodes) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    if (nodes != 0 && nodes < kSpectrumMinFrontier) {
        std::lock_guard<std::mutex> lock(bwt->mu);
        return fail(bwt, MSBWT_ERR_INVALID_ARG, "the spectrum frontier holds at least " + std::to_string(kSpectrumMinFrontier) + " nodes (0 = automatic)");
    }
    return set_locked(bwt, bwt->spectrum_frontier, nodes);
}

int msbwt_rle_spectrum_info(const msbwt_rle *bwt, uint64_t *out) {
    Call c(bwt);
    if (!c.h || !out) return MSBWT_ERR_INVALID_ARG;
    std::copy(c.h->spectrum_info, c.h->spectrum_info + MSBWT_SPECTRUM_INFO_WORDS, out);
    return MSBWT_OK;
}

int msbwt_spectrum_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, int sorted, uint64_t *device_bytes) {
    uint64_t bytes = 0;
    if (int rc = plan_bytes(total_rows, free_hbm_bytes, 0, records, sorted != 0, &bytes)) return rc;
    if (device_bytes) *device_bytes = bytes;
    return MSBWT_OK;
}

// ---- canonical k-mers: a k-mer and its reverse complement as one class ----

int msbwt_kmers_reverse_complement_2bit(const uint64_t *words, size_t k, size_t n, uint64_t *out) {
    if (k < 1 || k > kSpectrumMaxK || (n && (!words || !out))) return MSBWT_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i) out[i] = reverse_complement_2bit(words[i], uint32_t(k));
    return MSBWT_OK;
}

int msbwt_rle_canonical_kmer_spectrum(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_distinct, uint64_t *out_occurrences) {
    Call c(bwt);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, "canonical_kmer_spectrum needs 1 <= k <= 32");
    if (n_bins < 2 || !out_hist) return fail(h, MSBWT_ERR_INVALID_ARG, "canonical_kmer_spectrum needs a histogram of at least 2 bins");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    const Clock clock;
    uint64_t scratch_bytes = 0;
    SpectrumInfo info;
    info.k = k;
    uint64_t totals[kCanonicalTotalWords] = {};
    std::fill(out_hist, out_hist + n_bins, 0ull);
    if (h->totals.total != 0) {
        Scratch s;
        if (int rc = take_scratch(h, s, false, uint64_t(n_bins) * 8, "canonical_kmer_spectrum", true)) return rc;
        uint64_t *d_hist = nullptr;
        if (s.arena.take(&d_hist, uint64_t(n_bins) * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, "canonical_kmer_spectrum: " + std::to_string(uint64_t(n_bins) * 8) + " bytes of HBM needed for the histogram");
        }
        HIP_TRY(h, hipMemsetAsync(d_hist, 0, uint64_t(n_bins) * 8, h->stream));
        CanonicalSink sink{};
        sink.mode = kCanonicalHist;
        sink.min = 1;
        sink.max = ~0ull;
        sink.hist = reinterpret_cast<unsigned long long *>(d_hist);
        sink.n_bins = n_bins;
        if (int rc = canonical_walk(h, s, k, 1, sink, &info, h->stream, kHostFlags, totals)) return rc;
        HIP_TRY(h, hipMemcpyAsync(out_hist, d_hist, uint64_t(n_bins) * 8, hipMemcpyDeviceToHost, h->stream));
        if (int rc = status_of(h, h->stream, kHostFlags)) return rc;  // synchronises; the search's flags
        scratch_bytes = s.arena.taken;
    }
    if (out_distinct) *out_distinct = totals[kCanonicalClasses];
    if (out_occurrences) *out_occurrences = totals[kCanonicalOccurrences];
    record(h, info, clock, scratch_bytes);
    return MSBWT_OK;
}

int msbwt_rle_enumerate_canonical_kmers(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, uint64_t *out_kmers2bit, uint64_t *out_own,
                                        uint64_t *out_other, uint64_t capacity, uint64_t *out_n) {
    return enumerate_canonical(bwt, k, min_count, max_count, true, out_kmers2bit, out_own, out_other, capacity, out_n, nullptr, kHostFlags);
}

int msbwt_rle_enumerate_canonical_kmers_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, void *d_out_kmers2bit, void *d_out_own,
                                               void *d_out_other, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return enumerate_canonical(bwt, k, min_count, max_count, false, d_out_kmers2bit, d_out_own, d_out_other, capacity, out_n, static_cast<hipStream_t>(hip_stream),
                               kDeviceFlags);
}

int msbwt_canonical_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes) {
    uint64_t bytes = 0;
    if (int rc = plan_bytes(total_rows, free_hbm_bytes, 0, records, false, &bytes)) return rc;
    if (device_bytes) *device_bytes = bytes + spectrum_frontier_nodes(total_rows, free_hbm_bytes, 0) * kCanonicalStageBytes;
    return MSBWT_OK;
}

// ---- k-mers by source: one spectrum per input of a merged index, and the dump filtered by per-source counts ----

int msbwt_rle_kmer_spectrum_by_source(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_sharing, uint64_t *out_distinct,
                                      uint64_t *out_occurrences) {
    Call c(bwt);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    if (int rc = need_sources(h)) return rc;
    if (k < 1 || k > kSpectrumMaxK) return fail(h, MSBWT_ERR_INVALID_ARG, "kmer_spectrum_by_source needs 1 <= k <= 32");
    if (n_bins < 2 || !out_hist) return fail(h, MSBWT_ERR_INVALID_ARG, "kmer_spectrum_by_source needs histograms of at least 2 bins");
    if (int rc = c.bind()) return rc;
    if (int rc = ensure_runtime(h)) return rc;
    const Clock clock;
    uint64_t scratch_bytes = 0;
    SpectrumInfo info;
    info.k = k;
    const uint64_t S = h->sources.n_sources, hist_bytes = S * uint64_t(n_bins) * 8;
    uint64_t totals[kSourceTotalWords] = {};
    std::fill(out_hist, out_hist + S * n_bins, 0ull);
    if (h->totals.total != 0) {
        Scratch s;
        if (int rc = take_scratch(h, s, false, hist_bytes + kSourceSinkFixedBytes, "kmer_spectrum_by_source")) return rc;
        SourceFixed f;
        if (int rc = take_source_fixed(h, s, f, "kmer_spectrum_by_source")) return rc;
        uint64_t *d_hist = nullptr;
        if (s.arena.take(&d_hist, hist_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, "kmer_spectrum_by_source: " + std::to_string(hist_bytes) + " bytes of HBM needed for the histograms");
        }
        HIP_TRY(h, hipMemsetAsync(d_hist, 0, hist_bytes, h->stream));
        SourceSink sink{};
        sink.mode = kSourceSinkHist;
        sink.min_total = 1;
        sink.max_total = ~0ull;
        sink.hist = reinterpret_cast<unsigned long long *>(d_hist);
        sink.n_bins = n_bins;
        sink.flags = h->d_flags + kHostFlags;
        if (int rc = by_source_walk(h, s, f, k, 1, sink, &info, h->stream, totals)) return rc;
        HIP_TRY(h, hipMemcpyAsync(out_hist, d_hist, hist_bytes, hipMemcpyDeviceToHost, h->stream));
        if (int rc = status_of(h, h->stream, kHostFlags)) return rc;  // synchronises
        scratch_bytes = s.arena.taken;
    }
    for (uint64_t s = 0; s < S; ++s) {  // bin 0: the k-mers of the index that source s does not hold
        uint64_t *row = out_hist + s * n_bins, distinct = 0;
        for (size_t b = 1; b < n_bins; ++b) distinct += row[b];
        row[0] = info.nodes[k] - distinct;
        if (out_distinct) out_distinct[s] = distinct;
        if (out_occurrences) out_occurrences[s] = totals[kSourceOccurrences + s];
    }
    if (out_sharing) std::copy(totals + kSourceSharing, totals + kSourceSharing + S + 1, out_sharing);
    record(h, info, clock, scratch_bytes);
    return MSBWT_OK;
}

int msbwt_rle_enumerate_kmers_by_source(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts, uint64_t min_total, uint64_t max_total,
                                        int sorted, uint64_t *out_kmers2bit, uint64_t *out_counts, uint64_t *out_l, uint64_t capacity, uint64_t *out_n) {
    return enumerate_by_source(bwt, k, min_counts, max_counts, min_total, max_total, sorted, true, out_kmers2bit, out_counts, out_l, capacity, out_n, nullptr, kHostFlags);
}

int msbwt_rle_enumerate_kmers_by_source_device(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts, uint64_t min_total,
                                               uint64_t max_total, int sorted, void *d_out_kmers2bit, void *d_out_counts, void *d_out_l, uint64_t capacity,
                                               uint64_t *out_n, void *hip_stream) {
    return enumerate_by_source(bwt, k, min_counts, max_counts, min_total, max_total, sorted, false, d_out_kmers2bit, d_out_counts, d_out_l, capacity, out_n,
                               static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

// ---- the k-mer graph: an edge byte per k-mer of the sorted dump, and the table of (in, out) degrees ----

int msbwt_rle_enumerate_kmer_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_kmers2bit, uint64_t *out_counts, uint64_t *out_l,
                                   uint8_t *out_edges, uint64_t capacity, uint64_t *out_n) {
    return kmer_graph(bwt, k, min_count, min_edge, true, out_kmers2bit, out_counts, out_l, out_edges, capacity, out_n, nullptr, nullptr, nullptr, kHostFlags);
}

int msbwt_rle_enumerate_kmer_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_kmers2bit, void *d_out_counts, void *d_out_l,
                                          void *d_out_edges, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return kmer_graph(bwt, k, min_count, min_edge, false, d_out_kmers2bit, d_out_counts, d_out_l, d_out_edges, capacity, out_n, nullptr, nullptr,
                      static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

int msbwt_rle_kmer_graph_degrees(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_table, uint64_t *out_nodes, uint64_t *out_edges) {
    uint64_t unwanted[kGraphTableWords];
    return kmer_graph(bwt, k, min_count, min_edge, true, nullptr, nullptr, nullptr, nullptr, 0, out_nodes, out_table ? out_table : unwanted, out_edges, nullptr, kHostFlags);
}

int msbwt_kmer_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes) {
    uint64_t bytes = 0;
    if (int rc = graph_plan_bytes(total_rows, free_hbm_bytes, records, 3, &bytes)) return rc;
    if (device_bytes) *device_bytes = bytes;
    return MSBWT_OK;
}

int msbwt_rle_spectrum_scratch_bytes(const msbwt_rle *bwt, uint64_t *out_bytes) {
    Call c(bwt);
    if (!c.h || !out_bytes) return MSBWT_ERR_INVALID_ARG;
    *out_bytes = c.h->spectrum_scratch;
    return MSBWT_OK;
}

int msbwt_kmers_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, size_t n_sources, uint64_t records, int sorted, uint64_t *device_bytes) {
    uint64_t bytes = 0;
    if (int rc = by_source_plan_bytes(total_rows, free_hbm_bytes, 0, n_sources, records, sorted != 0, &bytes)) return rc;
    if (device_bytes) *device_bytes = bytes;
    return MSBWT_OK;
}

}  // extern "C"
