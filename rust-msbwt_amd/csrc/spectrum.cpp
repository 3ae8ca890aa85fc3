// The spectra and the k-mer dumps of a loaded index, three kinds of three calls each -- the abundance spectrum and the dump in its
// host and its device form: the plain k-mers (spectrum.hpp), a k-mer and its reverse complement as one class (canonical.hpp; the other
// strand is counted by query.cpp's packed search) and the k-mers by source of a merged index (source_spectrum.hpp).  Beside them what
// every walk call leaves on the handle or takes from it: the frontier setter, the info and scratch getters.  The kernels are behind
// those headers; the frame of a call is walk_call.hpp's, and a body here is its argument checks, its sink, and the order of its passes.
#include "walk_call.hpp"

#include "canonical.hpp"
#include "source_spectrum.hpp"

namespace {

Shape plain_shape(bool rank) { return Shape{rank, false, 0, kRecordBytes}; }
constexpr Shape kCanonicalShape{false, true, 0, kRecordBytes};  // (its totals, 256 bytes more, are in no plan)
Shape by_source_shape(bool rank, uint64_t n_sources) { return Shape{rank, false, kSourceSinkFixedBytes, (2 + n_sources) * sizeof(uint64_t)}; }

// a dump's own rung of the guard ladder: the window of counts, then its pointers
int dump_args(const Frame &f, uint64_t min_count, uint64_t max_count, const uint64_t *out_n, uint64_t capacity, const void *out_kmers) {
    if (max_count != 0 && min_count > max_count) return f.refuse(": min_count > max_count");
    return f.need_outputs(out_n, capacity, out_kmers);
}

// a spectrum's histograms in HBM, zeroed
int take_histogram(Frame &f, uint64_t bytes, const char *for_what, uint64_t **d_hist) {
    if (int rc = f.take(d_hist, bytes, f.needs(bytes, false, for_what))) return rc;
    HIP_TRY(f.h, hipMemsetAsync(*d_hist, 0, bytes, f.stream));
    return MSBWT_OK;
}

// A spectrum: out_hist (one histogram of n_bins bins, or one per source) zeroed, and on an index that holds something the scratch of
// `p` and the histograms taken, walk(bytes, &d_hist) -- which allocates the histograms (take_histogram) behind whatever else its sink
// needs, and walks -- and the histograms copied out; flags: the walk's kernels can flag, so the host flags are read.  Records the call.
template <class Walk>
int spectrum(Frame &f, bool sources, Shape p, bool flags, uint64_t *out_hist, size_t n_bins, Walk &&walk) {
    const char *too_few = sources ? " needs histograms of at least 2 bins" : " needs a histogram of at least 2 bins";
    if (int rc = f.open(sources, [&] { return n_bins < 2 || !out_hist ? f.refuse(too_few) : int(MSBWT_OK); })) return rc;
    msbwt_rle *h = f.h;
    const uint64_t words = (sources ? h->sources.n_sources : 1) * uint64_t(n_bins);
    std::fill(out_hist, out_hist + words, 0ull);
    if (!f.empty()) {
        p.fixed += words * 8;
        if (int rc = take_scratch(f, p)) return rc;
        uint64_t *d_hist = nullptr;
        if (int rc = walk(words * 8, &d_hist)) return rc;
        HIP_TRY(h, hipMemcpyAsync(out_hist, d_hist, words * 8, hipMemcpyDeviceToHost, f.stream));
        if (flags) {
            if (int rc = status_of(h, f.stream, f.which)) return rc;  // synchronises
        } else {
            HIP_TRY(h, hipStreamSynchronize(f.stream));
        }
        f.release();
    }
    f.record();
    return MSBWT_OK;
}

// ---- plain k-mers ----

// Both forms of the dump: records (k-mer, count, l).
int enumerate(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted, bool host, void *out_kmers, void *out_counts, void *out_l,
              uint64_t capacity, uint64_t *out_n, hipStream_t stream) {
    Frame f(bwt, "enumerate_kmers", k, host, stream);
    if (int rc = f.open(false, [&] { return dump_args(f, min_count, max_count, out_n, capacity, out_kmers); })) return rc;
    msbwt_rle *h = f.h;
    const IndexView v = view_of(h);
    const SpectrumSeeds seeds = seeds_of(f);
    Column cols[] = {{out_kmers}, {out_counts}, {out_l}};
    return two_pass(
        f, capacity, out_n, "k-mers", false,
        [&](uint64_t *n) -> int {
            if (int rc = take_scratch(f, plain_shape(sorted != 0 && capacity != 0))) return rc;
            HIP_TRY(h, spectrum_count(v, seeds, uint32_t(k), min_count, max_count, f.work, f.frontier, f.rank, n, &f.info, f.stream));
            return MSBWT_OK;
        },
        [&](uint64_t n) -> int {
            if (int rc = stage_records(f, cols, n, &capacity, "for the records")) return rc;
            HIP_TRY(h, spectrum_dump(v, seeds, uint32_t(k), min_count, max_count, f.work, f.frontier, f.rank, cols[0].as<uint64_t>(), cols[1].as<uint64_t>(),
                                     cols[2].as<uint64_t>(), capacity, h->d_flags + f.which, &f.info, f.stream));
            return MSBWT_OK;
        },
        [&](uint64_t) { return copy_out(f, cols); });
}

// ---- canonical k-mers ----

// Both forms of the canonical dump: records (canonical word, own, other), in the order the walk produces them.
int enumerate_canonical(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, bool host, void *out_kmers, void *out_own, void *out_other,
                        uint64_t capacity, uint64_t *out_n, hipStream_t stream) {
    Frame f(bwt, "enumerate_canonical_kmers", k, host, stream);
    if (int rc = f.open(false, [&] { return dump_args(f, min_count, max_count, out_n, capacity, out_kmers); })) return rc;
    CanonicalSink sink{};
    sink.mode = kCanonicalCount;
    sink.min = std::max<uint64_t>(min_count, 1);
    sink.max = max_count ? max_count : ~0ull;
    // of two strands whose counts sum to sink.min or more, the one that emits the class -- the larger -- has at least half of it
    const uint64_t prune = sink.min / 2 + sink.min % 2;
    uint64_t totals[kCanonicalTotalWords] = {};
    Column cols[] = {{out_kmers}, {out_own}, {out_other}};
    return two_pass(
        f, capacity, out_n, "classes", true,
        [&](uint64_t *n) -> int {
            if (int rc = take_scratch(f, kCanonicalShape)) return rc;
            if (int rc = canonical_walk(f, prune, sink, totals)) return rc;
            *n = totals[kCanonicalClasses];
            return MSBWT_OK;
        },
        [&](uint64_t n) -> int {
            if (int rc = stage_records(f, cols, n, &capacity, "for the records")) return rc;
            sink.mode = kCanonicalAppend;
            sink.kmers = cols[0].as<uint64_t>();
            sink.own = cols[1].as<uint64_t>();
            sink.other = cols[2].as<uint64_t>();
            sink.capacity = capacity;
            sink.flags = f.h->d_flags + f.which;
            return canonical_walk(f, prune, sink, totals);
        },
        [&](uint64_t) { return copy_out(f, cols); });
}

// ---- k-mers by source ----

// the sink's fixed words: the limits, then the totals
struct SourceFixed {
    uint64_t *limits = nullptr;
    unsigned long long *totals = nullptr;
};

int take_source_fixed(Frame &f, SourceFixed &x) {
    if (int rc = f.take(&x.limits, kSourceSinkFixedBytes, f.needs(kSourceSinkFixedBytes, true, "for the sink"))) return rc;
    x.totals = reinterpret_cast<unsigned long long *>(x.limits + 2 * kSourceMax);
    return MSBWT_OK;
}

// One walk of a by-source call: a chunk's k-mers go to the source sink (its totals: x.totals, copied to totals[] at the end).
// Synchronises the stream.
int by_source_walk(Frame &f, const SourceFixed &x, uint64_t prune, SourceSink sink, uint64_t *totals) {
    sink.totals = x.totals;
    sink.limits = x.limits;
    const SourceView view = f.h->sources.view(f.h->totals.total);
    return staged_walk(f, prune, x.totals, kSourceTotalWords, totals, [&](const void *d_kmers, uint64_t m) { return launch_source_sink(d_kmers, m, view, sink, f.stream); });
}

uint64_t add_saturating(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// Both forms of the by-source dump: records (word, c_0 .. c_{S-1}, l).
int enumerate_by_source(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts, uint64_t min_total, uint64_t max_total, int sorted, bool host,
                        void *out_kmers, void *out_counts, void *out_l, uint64_t capacity, uint64_t *out_n, hipStream_t stream) {
    Frame f(bwt, "enumerate_kmers_by_source", k, host, stream);
    uint64_t limits[2 * kSourceMax];
    uint64_t min_sum = 0;
    if (int rc = f.open(true, [&] {
            const uint64_t S = f.h->sources.n_sources;
            for (uint32_t s = 0; s < kSourceMax; ++s) {
                limits[s] = s < S && min_counts ? min_counts[s] : 0ull;
                limits[kSourceMax + s] = s < S && max_counts ? max_counts[s] : ~0ull;
                if (limits[s] > limits[kSourceMax + s]) return f.refuse(": min_counts[" + std::to_string(s) + "] > max_counts[" + std::to_string(s) + "]");
                min_sum = add_saturating(min_sum, limits[s]);
            }
            if (max_total != 0 && min_total > max_total) return f.refuse(": min_total > max_total");
            return f.need_outputs(out_n, capacity, out_kmers);
        }))
        return rc;
    msbwt_rle *h = f.h;
    // a suffix's total is at least the k-mer's, and the k-mer's is at least the sum of its minima
    const uint64_t prune = std::max(std::max<uint64_t>(min_total, 1), min_sum);
    const bool rank = sorted != 0 && capacity != 0;
    SourceFixed x;
    SourceSink sink{};
    sink.mode = kSourceSinkCount;
    sink.min_total = std::max<uint64_t>(min_total, 1);
    sink.max_total = max_total ? max_total : ~0ull;
    SpectrumRank r{};
    uint64_t totals[kSourceTotalWords] = {};
    Column cols[] = {{out_kmers}, {out_counts, 8 * h->sources.n_sources}, {out_l}};
    return two_pass(
        f, capacity, out_n, "k-mers", true,
        [&](uint64_t *n) -> int {
            if (int rc = take_scratch(f, by_source_shape(rank, h->sources.n_sources))) return rc;
            if (int rc = take_source_fixed(f, x)) return rc;
            HIP_TRY(h, hipMemcpyAsync(x.limits, limits, sizeof limits, hipMemcpyHostToDevice, f.stream));
            HIP_TRY(h, hipStreamSynchronize(f.stream));  // (the limits are this frame's)
            sink.flags = h->d_flags + f.which;
            if (rank) {
                r = spectrum_rank_view(f.rank, h->totals.total);
                HIP_TRY(h, spectrum_rank_clear(r, f.stream));
                sink.bitmap = r.bitmap;
            }
            if (int rc = by_source_walk(f, x, prune, sink, totals)) return rc;
            *n = totals[kSourcePassed];
            return MSBWT_OK;
        },
        [&](uint64_t n) -> int {
            sink.mode = rank ? kSourceSinkScatter : kSourceSinkAppend;
            if (rank) {
                HIP_TRY(h, spectrum_rank_close(r, f.stream));
                sink.prefix = r.prefix;
            }
            if (int rc = stage_records(f, cols, n, &capacity, "for the records")) return rc;
            sink.kmers = cols[0].as<uint64_t>();
            sink.counts = cols[1].as<uint64_t>();
            sink.l = cols[2].as<uint64_t>();
            sink.capacity = capacity;
            return by_source_walk(f, x, prune, sink, totals);
        },
        [&](uint64_t) { return copy_out(f, cols); });
}

}  // namespace

extern "C" {

int msbwt_rle_kmer_spectrum(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_distinct, uint64_t *out_occurrences) {
    Frame f(bwt, "kmer_spectrum", k);
    uint64_t distinct = 0, occurrences = 0;
    if (int rc = spectrum(f, false, plain_shape(false), false, out_hist, n_bins, [&](uint64_t bytes, uint64_t **d_hist) -> int {
            if (int rc = take_histogram(f, bytes, "for the histogram", d_hist)) return rc;
            HIP_TRY(f.h, spectrum_histogram(view_of(f.h), seeds_of(f), uint32_t(k), f.work, f.frontier, *d_hist, n_bins, &distinct, &occurrences, &f.info, f.stream));
            return MSBWT_OK;
        }))
        return rc;
    if (out_distinct) *out_distinct = distinct;
    if (out_occurrences) *out_occurrences = occurrences;
    return MSBWT_OK;
}

int msbwt_rle_enumerate_kmers(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted, uint64_t *out_kmers2bit, uint64_t *out_counts,
                              uint64_t *out_l, uint64_t capacity, uint64_t *out_n) {
    return enumerate(bwt, k, min_count, max_count, sorted, true, out_kmers2bit, out_counts, out_l, capacity, out_n, nullptr);
}

int msbwt_rle_enumerate_kmers_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted, void *d_out_kmers2bit, void *d_out_counts,
                                     void *d_out_l, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return enumerate(bwt, k, min_count, max_count, sorted, false, d_out_kmers2bit, d_out_counts, d_out_l, capacity, out_n, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_set_spectrum_frontier(msbwt_rle *bwt, uint64_t nodes) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    if (nodes != 0 && nodes < kSpectrumMinFrontier) {
        std::lock_guard<std::mutex> lock(bwt->mu);
        return fail(bwt, MSBWT_ERR_INVALID_ARG, "the spectrum frontier holds at least " + std::to_string(kSpectrumMinFrontier) + " nodes (0 = automatic)");
    }
    return set_locked(bwt, bwt->spectrum_frontier, nodes);
}

int msbwt_rle_spectrum_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::spectrum_info, out); }

int msbwt_rle_spectrum_scratch_bytes(const msbwt_rle *bwt, uint64_t *out_bytes) {
    Call c(bwt);
    if (!c.h || !out_bytes) return MSBWT_ERR_INVALID_ARG;
    *out_bytes = c.h->spectrum_scratch;
    return MSBWT_OK;
}

int msbwt_spectrum_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, int sorted, uint64_t *device_bytes) {
    return plan(plain_shape(sorted != 0), total_rows, free_hbm_bytes, records, 0, device_bytes);
}

// ---- canonical k-mers: a k-mer and its reverse complement as one class ----

int msbwt_kmers_reverse_complement_2bit(const uint64_t *words, size_t k, size_t n, uint64_t *out) {
    if (k < 1 || k > kSpectrumMaxK || (n && (!words || !out))) return MSBWT_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i) out[i] = reverse_complement_2bit(words[i], uint32_t(k));
    return MSBWT_OK;
}

int msbwt_rle_canonical_kmer_spectrum(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_distinct, uint64_t *out_occurrences) {
    Frame f(bwt, "canonical_kmer_spectrum", k);
    uint64_t totals[kCanonicalTotalWords] = {};
    if (int rc = spectrum(f, false, kCanonicalShape, true, out_hist, n_bins, [&](uint64_t bytes, uint64_t **d_hist) -> int {  // (flags: the search's)
            if (int rc = take_histogram(f, bytes, "for the histogram", d_hist)) return rc;
            CanonicalSink sink{};
            sink.mode = kCanonicalHist;
            sink.min = 1;
            sink.max = ~0ull;
            sink.hist = reinterpret_cast<unsigned long long *>(*d_hist);
            sink.n_bins = n_bins;
            return canonical_walk(f, 1, sink, totals);
        }))
        return rc;
    if (out_distinct) *out_distinct = totals[kCanonicalClasses];
    if (out_occurrences) *out_occurrences = totals[kCanonicalOccurrences];
    return MSBWT_OK;
}

int msbwt_rle_enumerate_canonical_kmers(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, uint64_t *out_kmers2bit, uint64_t *out_own,
                                        uint64_t *out_other, uint64_t capacity, uint64_t *out_n) {
    return enumerate_canonical(bwt, k, min_count, max_count, true, out_kmers2bit, out_own, out_other, capacity, out_n, nullptr);
}

int msbwt_rle_enumerate_canonical_kmers_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, void *d_out_kmers2bit, void *d_out_own,
                                               void *d_out_other, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return enumerate_canonical(bwt, k, min_count, max_count, false, d_out_kmers2bit, d_out_own, d_out_other, capacity, out_n, static_cast<hipStream_t>(hip_stream));
}

int msbwt_canonical_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes) {
    return plan(kCanonicalShape, total_rows, free_hbm_bytes, records, 0, device_bytes);
}

// ---- k-mers by source: one spectrum per input of a merged index, and the dump filtered by per-source counts ----

int msbwt_rle_kmer_spectrum_by_source(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_sharing, uint64_t *out_distinct,
                                      uint64_t *out_occurrences) {
    Frame f(bwt, "kmer_spectrum_by_source", k);
    uint64_t totals[kSourceTotalWords] = {};
    if (int rc = spectrum(f, true, by_source_shape(false, f.h ? f.h->sources.n_sources : 0), true, out_hist, n_bins, [&](uint64_t bytes, uint64_t **d_hist) -> int {
            SourceFixed x;
            if (int rc = take_source_fixed(f, x)) return rc;
            if (int rc = take_histogram(f, bytes, "for the histograms", d_hist)) return rc;
            SourceSink sink{};
            sink.mode = kSourceSinkHist;
            sink.min_total = 1;
            sink.max_total = ~0ull;
            sink.hist = reinterpret_cast<unsigned long long *>(*d_hist);
            sink.n_bins = n_bins;
            sink.flags = f.h->d_flags + f.which;
            return by_source_walk(f, x, 1, sink, totals);
        }))
        return rc;
    const uint64_t S = f.h->sources.n_sources;
    for (uint64_t s = 0; s < S; ++s) {  // bin 0: the k-mers of the index that source s does not hold
        uint64_t *row = out_hist + s * n_bins, distinct = 0;
        for (size_t b = 1; b < n_bins; ++b) distinct += row[b];
        row[0] = f.info.nodes[k] - distinct;
        if (out_distinct) out_distinct[s] = distinct;
        if (out_occurrences) out_occurrences[s] = totals[kSourceOccurrences + s];
    }
    if (out_sharing) std::copy(totals + kSourceSharing, totals + kSourceSharing + S + 1, out_sharing);
    return MSBWT_OK;
}

int msbwt_rle_enumerate_kmers_by_source(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts, uint64_t min_total, uint64_t max_total,
                                        int sorted, uint64_t *out_kmers2bit, uint64_t *out_counts, uint64_t *out_l, uint64_t capacity, uint64_t *out_n) {
    return enumerate_by_source(bwt, k, min_counts, max_counts, min_total, max_total, sorted, true, out_kmers2bit, out_counts, out_l, capacity, out_n, nullptr);
}

int msbwt_rle_enumerate_kmers_by_source_device(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts, uint64_t min_total,
                                               uint64_t max_total, int sorted, void *d_out_kmers2bit, void *d_out_counts, void *d_out_l, uint64_t capacity,
                                               uint64_t *out_n, void *hip_stream) {
    return enumerate_by_source(bwt, k, min_counts, max_counts, min_total, max_total, sorted, false, d_out_kmers2bit, d_out_counts, d_out_l, capacity, out_n,
                               static_cast<hipStream_t>(hip_stream));
}

int msbwt_kmers_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, size_t n_sources, uint64_t records, int sorted, uint64_t *device_bytes) {
    if (n_sources < 1 || n_sources > kSourceMax) return MSBWT_ERR_INVALID_ARG;
    return plan(by_source_shape(sorted != 0, n_sources), total_rows, free_hbm_bytes, records, 0, device_bytes);
}

}  // extern "C"
