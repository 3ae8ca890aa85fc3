// The k-mer walk calls of a loaded index, six families.  Four of three calls each -- the abundance spectrum, the k-mer dump in its host
// and its device form (the graph: and the degree table): the plain k-mers (spectrum.hpp), a k-mer and its reverse complement as one
// class (canonical.hpp; the other strand is counted by query.cpp's packed search), the k-mers by source of a merged index
// (source_spectrum.hpp) and the k-mer graph (kmer_graph.hpp).  Two of two, a host and a device form: the unitigs that graph compacts
// into (unitigs.hpp: the graph's walks into scratch, then kernels over its slots) and the canonical unitigs (canonical_unitigs.hpp: the
// same compaction over both members of every canonical class), each also as a unitig GRAPH call that adds the link table of the
// compacted graph behind the emission (unitig_links.hpp), and that once more by source: the matrix of per-input sums behind the links
// (unitig_sources.hpp).  Beside them the traces (trace.hpp): no walk of the index but rounds of the packed search over the live walks of a
// batch of seeds, in the same frame.  The kernels are behind those headers; this file is the host side, and
// what the calls share is written once:
//   Frame         a call: the locked handle, the guard ladder (no index, no sources, k, the call's own arguments, the device), the
//                 stream, the clock, the SpectrumInfo and the scratch -- allocated per call, freed before it returns -- and, built from
//                 the one name the call passes, every text it can say
//   Shape         what a family allocates: its msbwt_*_plan and the sufficiency check of take_scratch are the same sum over it
//   layouts       graph_layouts.hpp: where the arrays of the graph's and the unitigs' blocks lie -- the plan takes a layout's bytes, the
//                 call carves base + field, the memset runs over the span it names; nothing here adds up a block of its own
//   two_pass      a dump: the counting pass, *out_n, the capacity pattern, the filling pass, the record after either
//   stage_records / copy_out   the columns of a dump: the caller's device arrays, or one staged block carved up and copied out
//   staged_walk   a walk whose chunks go to a sink behind it (canonical, by source, the graph's edge pass)
//   spectrum      a spectrum: the histograms zeroed, taken, walked into and copied out
//   GraphCut / graph_edge_walk   the thresholds of the three graph calls and their staged walk with the edge pass behind it
//   rank_unitigs / UnitigOutputs   the compaction both unitig calls run over their slots, and their outputs from guard to delivery;
//                 UnitigLinkOutputs: the link table the unitig graph calls add behind the emission (unitig_links.hpp)
//                 UnitigSourceOutputs: the matrix by source the by-source graph calls add behind the links (unitig_sources.hpp)
// A body below is what is left: its argument checks, its sink, and the order of its passes.
#include <algorithm>
#include <chrono>
#include <string>

#include "canonical.hpp"
#include "canonical_unitigs.hpp"
#include "graph_layouts.hpp"
#include "handle.hpp"
#include "kmer_graph.hpp"
#include "order.hpp"
#include "radix_sort.hpp"
#include "run_encode.hpp"
#include "source_spectrum.hpp"
#include "spectrum.hpp"
#include "trace.hpp"
#include "unitig_links.hpp"
#include "unitig_sources.hpp"
#include "unitigs.hpp"

namespace {

static_assert(MSBWT_SPECTRUM_MIN_FRONTIER == kSpectrumMinFrontier && MSBWT_SPECTRUM_INFO_WORDS == 4 + kSpectrumMaxK + 1 + 3, "the header's constants");
constexpr uint64_t kRecordBytes = 3 * sizeof(uint64_t);  // k-mer, count, l

// ---- what a family allocates ----

// The scratch of a call beyond the walk's own frontiers.  A plan counts `record_bytes` per record staged for a host dump; the call
// itself stages only the columns its caller wants.
struct Shape {
    bool rank;              // the bitmap over the rows and its checkpoints: a sorted call that fills buffers
    bool canonical;         // kCanonicalStageBytes per frontier node: the other strand of a chunk's k-mers
    uint64_t fixed;         // the sink's words, the histograms
    uint64_t record_bytes;
};

Shape plain_shape(bool rank) { return Shape{rank, false, 0, kRecordBytes}; }
constexpr Shape kCanonicalShape{false, true, 0, kRecordBytes};  // (its totals, 256 bytes more, are in no plan)
Shape by_source_shape(bool rank, uint64_t n_sources) { return Shape{rank, false, kSourceSinkFixedBytes, (2 + n_sources) * sizeof(uint64_t)}; }
Shape graph_shape(bool fill) { return Shape{fill, false, fill ? graph_tail_layout(0).bytes : 0, kRecordBytes}; }  // (fixed: the tail of no records)

uint64_t shape_bytes(const Shape &p, uint64_t total_rows, uint64_t frontier, uint64_t records) {
    return spectrum_work_bytes(frontier) + (p.rank ? spectrum_rank_bytes(total_rows) : 0) + (p.canonical ? frontier * kCanonicalStageBytes : 0) + p.fixed +
           records * p.record_bytes;
}

// a msbwt_*_plan: the shape at the automatic frontier, and `more`; MSBWT_ERR_TOO_LARGE for what no index can be
int plan(const Shape &p, uint64_t total_rows, uint64_t free_bytes, uint64_t records, uint64_t more, uint64_t *device_bytes) {
    if (total_rows >= kMaxSymbols || records >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) *device_bytes = shape_bytes(p, total_rows, spectrum_frontier_nodes(total_rows, free_bytes, 0), records) + more;
    return MSBWT_OK;
}

// ---- a call ----

struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    uint64_t us() const { return uint64_t(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count()); }
};

struct Frame {
    Call c;
    msbwt_rle *const h;
    const std::string name;  // as the texts say it: "enumerate_kmers"
    const size_t k;
    const bool host;         // the outputs are host arrays, and the call runs on the handle's stream and reads its flags before it returns
    hipStream_t stream;
    const int which;         // the word of the status block its kernels flag: the host forms', or the device forms'
    Clock clock;
    SpectrumInfo info;
    // the scratch, freed with the frame
    Arena arena;
    void *work = nullptr, *rank = nullptr;
    uint64_t frontier = 0;
    uint64_t *rc_words = nullptr, *rc_counts = nullptr;  // canonical calls: the other strand of a chunk's k-mers, `frontier` words each
    unsigned long long *totals = nullptr;                // and the words of CanonicalSink::totals
    int hook_rc = MSBWT_OK;                              // what a chunk hook's own call returned (staged_walk)

    // a host form (nullptr: the handle's stream, once open), or the device form on the caller's stream
    Frame(const msbwt_rle *bwt, const char *name, size_t k, bool host = true, hipStream_t stream = nullptr)
        : c(bwt), h(c.h), name(name), k(k), host(host), stream(stream), which(host ? kHostFlags : kDeviceFlags) {}

    int refuse(const std::string &why) const { return fail(h, MSBWT_ERR_INVALID_ARG, name + why); }
    // a dump's pointers: out_n always, the k-mers once there is a capacity
    int need_outputs(const uint64_t *out_n, uint64_t capacity, const void *out_kmers) const {
        return !out_n || (capacity && !out_kmers) ? fail(h, MSBWT_ERR_INVALID_ARG, host ? "null pointer" : "null device pointer") : int(MSBWT_OK);
    }

    // The guard ladder: no handle, no index, (sources wanted) none attached, k, the call's own arguments -- args() refuses or returns
    // MSBWT_OK --, the device.  From here on the clock runs.
    template <class Args>
    int open(bool sources, Args &&args) {
        if (!h) return MSBWT_ERR_INVALID_ARG;
        if (int rc = c.loaded()) return rc;
        if (sources && !h->sources.n_sources) return fail(h, MSBWT_ERR_NOT_LOADED, "no sources attached");
        if (k < 1 || k > kSpectrumMaxK) return refuse(" needs 1 <= k <= 32");
        if (int rc = args()) return rc;
        if (int rc = c.bind()) return rc;
        if (int rc = ensure_runtime(h)) return rc;
        if (host) stream = h->stream;
        clock = Clock{};
        info.k = k;
        return MSBWT_OK;
    }
    bool empty() const { return h->totals.total == 0; }  // nothing to walk: the call returns zeros, having allocated nothing

    // what the walks so far did, the time since open() and the scratch taken: msbwt_rle_spectrum_info, msbwt_rle_spectrum_scratch_bytes
    void record() {
        h->spectrum_scratch = arena.taken;
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
    void release() {  // the scratch given back before the frame goes (a spectrum: before it records)
        for (void *p : arena.held) (void)hipFree(p);
        arena.held.clear();
    }

    // the text of an allocation that failed or would: the call, the bytes, "more" for one on top of the scratch, and what for
    std::string needs(uint64_t bytes, bool more, const char *for_what) const {
        return name + ": " + std::to_string(bytes) + (more ? " more" : "") + " bytes of HBM needed " + for_what;
    }
    // One more allocation, or MSBWT_ERR_HIP saying `or_say`; ask_free: refused already where the device says it has less free.
    template <class T>
    int take(T **p, uint64_t bytes, const std::string &or_say, bool ask_free = false) {
        size_t free_bytes = ~size_t(0), all_bytes = 0;
        if (ask_free) HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
        if (free_bytes < bytes || arena.take(p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MSBWT_ERR_HIP, or_say);
        }
        return MSBWT_OK;
    }
    // a block on top of the scratch, asked for only where the device says it has that much free
    int take_more(char **block, uint64_t bytes, const char *for_what) { return take(block, bytes, needs(bytes, true, for_what), true); }
};

// where the walk starts: the flat direct table when it is shallower than k, else the root
SpectrumSeeds seeds_of(const Frame &f) {
    const DirectTable &t = f.h->table;
    if (t.entries && !t.packed && t.depth > 0 && size_t(t.depth) < f.k) return SpectrumSeeds{t.entries, t.depth};
    return SpectrumSeeds{};
}

// The frontiers and what else of `p` does not wait for the records (the rank scratch, the canonical staging and totals) in HBM, or
// MSBWT_ERR_HIP naming the bytes of the shape.  p.fixed is checked for here and taken by the call.
int take_scratch(Frame &f, const Shape &p) {
    msbwt_rle *h = f.h;
    size_t free_bytes = 0, all_bytes = 0;
    HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
    const uint64_t total = h->totals.total;
    f.frontier = spectrum_frontier_nodes(total, free_bytes, h->spectrum_frontier);
    const uint64_t bytes = shape_bytes(p, total, f.frontier, 0);
    const std::string need = f.needs(bytes, false, "while it runs");
    if (free_bytes < bytes) return fail(h, MSBWT_ERR_HIP, need);
    if (int rc = f.take(&f.work, spectrum_work_bytes(f.frontier), need)) return rc;
    if (p.rank)
        if (int rc = f.take(&f.rank, spectrum_rank_bytes(total), need)) return rc;
    if (p.canonical) {
        if (int rc = f.take(&f.rc_words, f.frontier * 8, need)) return rc;
        if (int rc = f.take(&f.rc_counts, f.frontier * 8, need)) return rc;
        if (int rc = f.take(&f.totals, kCanonicalTotalWords * 8, need)) return rc;
    }
    return MSBWT_OK;
}

// a spectrum's histograms in HBM, zeroed
int take_histogram(Frame &f, uint64_t bytes, const char *for_what, uint64_t **d_hist) {
    if (int rc = f.take(d_hist, bytes, f.needs(bytes, false, for_what))) return rc;
    HIP_TRY(f.h, hipMemsetAsync(*d_hist, 0, bytes, f.stream));
    return MSBWT_OK;
}

// ---- the records of a dump ----

// A column of a dump's records: the caller's array (`out`: of the host or of the device, as the frame says; nullptr = not wanted) of
// `words` 64-bit words per record, and where the sink writes it (`at`).
struct Column {
    void *out;
    uint64_t words = 1;
    uint64_t *at = nullptr;
};

// Where the sink writes: a device form's columns are the caller's own; a host form's are carved from one allocation of the n records'
// wanted words -- *capacity becomes n --, `tail_bytes` more behind them in either form (*tail).  Nothing to stage and no tail: no allocation.
template <size_t N>
int stage_records(Frame &f, Column (&cols)[N], uint64_t n, uint64_t *capacity, const char *for_what, uint64_t tail_bytes = 0, char **tail = nullptr) {
    uint64_t words = 0;
    for (Column &c : cols) {
        c.at = static_cast<uint64_t *>(c.out);
        if (f.host && c.out) words += c.words;
    }
    const uint64_t bytes = n * words * 8 + tail_bytes;
    if (bytes == 0) return MSBWT_OK;
    char *block = nullptr;
    if (int rc = f.take_more(&block, bytes, for_what)) return rc;
    if (tail) *tail = block + n * words * 8;
    if (!f.host) return MSBWT_OK;
    uint64_t *next = reinterpret_cast<uint64_t *>(block);
    for (Column &c : cols)
        if (c.out) {
            c.at = next;
            next += n * c.words;
        }
    *capacity = n;
    return MSBWT_OK;
}

// A host form's wanted columns copied out, and the flags its kernels left (synchronises).  A device form has its records where they
// belong, and a fault is in the device status word: msbwt_rle_device_status.
template <size_t N>
int copy_out(Frame &f, const Column (&cols)[N], uint64_t n) {
    if (!f.host) return MSBWT_OK;
    for (const Column &c : cols)
        if (c.out) HIP_TRY(f.h, hipMemcpyAsync(c.out, c.at, n * c.words * 8, hipMemcpyDeviceToHost, f.stream));
    return status_of(f.h, f.stream, f.which);
}

// ---- the passes ----

// A dump, or any call of the two-call pattern.  count(&n) walks once and says how many records qualify: *out_n (which only the degree
// table leaves out).  capacity 0, or nothing qualifies: that was the call (a host form whose counting pass can flag -- flags_after_count
// -- reads the flags first); a capacity below n is refused; else fill(n) walks again, into the buffers, and deliver(n) hands them over
// once the walk is recorded.  `things`: what qualifies, for the refusal.
template <class Count, class Fill, class Deliver>
int two_pass(Frame &f, uint64_t capacity, uint64_t *out_n, const char *things, bool flags_after_count, Count &&count, Fill &&fill, Deliver &&deliver) {
    if (out_n) *out_n = 0;
    if (f.empty()) {
        f.record();
        return MSBWT_OK;
    }
    uint64_t n = 0;
    if (int rc = count(&n)) return rc;
    if (out_n) *out_n = n;
    f.record();
    if (capacity == 0 || n == 0) return flags_after_count && f.host ? status_of(f.h, f.stream, f.which) : int(MSBWT_OK);
    if (capacity < n) return f.refuse(": capacity " + std::to_string(capacity) + " is less than the n = " + std::to_string(n) + " " + things + " that qualify");
    if (int rc = fill(n)) return rc;
    f.record();
    return deliver(n);
}

// One staged walk: chunk by chunk the k-mers at least `prune` wide are staged and handed to per_chunk, which launches the sink.  The
// sink's totals (`words` of them at d_totals; nullptr: it has none) are zeroed before and copied to totals[] after, and then the stream
// is synchronised.  A hook that fails in a call of its own leaves that call's code in f.hook_rc, which wins over the walk's error.
int staged_walk(Frame &f, uint64_t prune, unsigned long long *d_totals, uint32_t words, uint64_t *totals, const SpectrumChunkHook &per_chunk) {
    msbwt_rle *h = f.h;
    f.hook_rc = MSBWT_OK;
    if (d_totals) HIP_TRY(h, hipMemsetAsync(d_totals, 0, words * 8, f.stream));
    const hipError_t walked = spectrum_stage(view_of(h), seeds_of(f), uint32_t(f.k), prune, f.work, f.frontier, per_chunk, &f.info, f.stream);
    if (f.hook_rc) return f.hook_rc;
    HIP_TRY(h, walked);
    if (!d_totals) return MSBWT_OK;
    HIP_TRY(h, hipMemcpyAsync(totals, d_totals, words * 8, hipMemcpyDeviceToHost, f.stream));
    HIP_TRY(h, hipStreamSynchronize(f.stream));
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
    if (int rc = f.open(false, [&] {
            if (max_count != 0 && min_count > max_count) return f.refuse(": min_count > max_count");
            return f.need_outputs(out_n, capacity, out_kmers);
        }))
        return rc;
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
            HIP_TRY(h, spectrum_dump(v, seeds, uint32_t(k), min_count, max_count, f.work, f.frontier, f.rank, cols[0].at, cols[1].at, cols[2].at, capacity,
                                     h->d_flags + f.which, &f.info, f.stream));
            return MSBWT_OK;
        },
        [&](uint64_t n) { return copy_out(f, cols, n); });
}

// ---- canonical k-mers ----

// One walk of a canonical call: the reverse complements of a chunk's k-mers are written as packed words and counted by the packed
// search, and the classes they emit go to `sink` (its totals: f.totals, copied to totals[] at the end).  Synchronises the stream.
int canonical_walk(Frame &f, uint64_t prune, CanonicalSink sink, uint64_t *totals) {
    sink.totals = f.totals;
    return staged_walk(f, prune, f.totals, kCanonicalTotalWords, totals, [&](const void *d_kmers, uint64_t m) {
        const hipError_t e = launch_canonical_rc(d_kmers, m, uint32_t(f.k), f.rc_words, f.stream);
        if (e != hipSuccess) return e;
        if ((f.hook_rc = launch_count_2bit(f.h, f.rc_words, f.k, size_t(m), f.rc_counts, f.stream, f.which)) != MSBWT_OK) return hipErrorUnknown;
        return launch_canonical_combine(d_kmers, f.rc_words, f.rc_counts, m, sink, f.stream);
    });
}

// Both forms of the canonical dump: records (canonical word, own, other), in the order the walk produces them.
int enumerate_canonical(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, bool host, void *out_kmers, void *out_own, void *out_other,
                        uint64_t capacity, uint64_t *out_n, hipStream_t stream) {
    Frame f(bwt, "enumerate_canonical_kmers", k, host, stream);
    if (int rc = f.open(false, [&] {
            if (max_count != 0 && min_count > max_count) return f.refuse(": min_count > max_count");
            return f.need_outputs(out_n, capacity, out_kmers);
        }))
        return rc;
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
            sink.kmers = cols[0].at;
            sink.own = cols[1].at;
            sink.other = cols[2].at;
            sink.capacity = capacity;
            sink.flags = f.h->d_flags + f.which;
            return canonical_walk(f, prune, sink, totals);
        },
        [&](uint64_t n) { return copy_out(f, cols, n); });
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
    Column cols[] = {{out_kmers}, {out_counts, h->sources.n_sources}, {out_l}};
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
            sink.kmers = cols[0].at;
            sink.counts = cols[1].at;
            sink.l = cols[2].at;
            sink.capacity = capacity;
            return by_source_walk(f, x, prune, sink, totals);
        },
        [&](uint64_t n) { return copy_out(f, cols, n); });
}

// ---- the k-mer graph ----

// What the graph and both unitig calls take for a node and for an edge: a k-mer at least m wide, a (k+1)-mer at least me.
struct GraphCut {
    uint64_t m, me;
    GraphCut(uint64_t min_count, uint64_t min_edge) : m(std::max<uint64_t>(min_count, 1)), me(min_edge ? min_edge : m) {}
    // the calls' own rung of the guard ladder: the thresholds, then the output no call can do without
    int check(const Frame &f, const void *needed) const {
        if (me < m) return f.refuse(": min_edge is below the node threshold (0 = the node threshold)");
        return !needed ? fail(f.h, MSBWT_ERR_INVALID_ARG, "null pointer") : int(MSBWT_OK);
    }
};

// an array of a block, at the offset its layout gives (graph_layouts.hpp)
template <class T>
T *in(char *block, uint64_t offset) {
    return reinterpret_cast<T *>(block + offset);
}

// the sorted dump's counting walk: the scratch of `p`, *n = the nodes, and with p.rank the bit of every node's l
int count_nodes(Frame &f, const Shape &p, const GraphCut &cut, uint64_t *n) {
    if (int rc = take_scratch(f, p)) return rc;
    HIP_TRY(f.h, spectrum_count(view_of(f.h), seeds_of(f), uint32_t(f.k), cut.m, 0, f.work, f.frontier, f.rank, n, &f.info, f.stream));
    return MSBWT_OK;
}

// The staged walk with the edge pass behind it: the n nodes' columns (each optional) at the rank of their l, their edge bytes ORed into
// edge_words (zeroed by the caller) and, where pred is given, the slot of a predecessor.
int graph_edge_walk(Frame &f, const GraphCut &cut, uint64_t n, uint32_t *edge_words, uint64_t *kmers, uint64_t *counts, uint64_t *l, uint64_t *pred) {
    const IndexView v = view_of(f.h);
    const SpectrumRank r = spectrum_rank_view(f.rank, f.h->totals.total);
    const GraphSink sink{r.bitmap, r.prefix, edge_words, n, cut.me, kmers, counts, l, f.h->d_flags + f.which, pred};
    return staged_walk(f, cut.m, nullptr, 0, nullptr, [&](const void *d_nodes, uint64_t nodes) { return launch_graph_edges(v, d_nodes, nodes, sink, f.stream); });
}

// The dump (both forms) and the degree table (table != nullptr: no record outputs, *out_n = the nodes, *out_edge_count = the edges):
// the sorted dump's counting walk, then the staged walk with the edge pass behind it.
int kmer_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, bool host, void *out_kmers, void *out_counts, void *out_l, void *out_edges,
               uint64_t capacity, uint64_t *out_n, uint64_t *table, uint64_t *out_edge_count, hipStream_t stream) {
    const bool degrees = table != nullptr;
    Frame f(bwt, degrees ? "kmer_graph_degrees" : "enumerate_kmer_graph", k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = f.open(false, [&] { return cut.check(f, degrees ? table : out_n); })) return rc;
    msbwt_rle *h = f.h;
    if (out_edge_count) *out_edge_count = 0;
    if (degrees) std::fill(table, table + kGraphTableWords, 0ull);
    const bool fill = degrees || capacity != 0;  // (the degree table has no capacity to fall short)
    Column cols[] = {{out_kmers}, {out_counts}, {out_l}};
    GraphTailLayout at{};
    char *tail = nullptr;
    return two_pass(
        f, degrees ? ~0ull : capacity, out_n, "k-mers", false, [&](uint64_t *n) { return count_nodes(f, graph_shape(fill), cut, n); },
        [&](uint64_t n) -> int {
            // one allocation: the records staged for a host dump, and graph_tail_layout behind them
            at = graph_tail_layout(n);
            if (int rc = stage_records(f, cols, n, &capacity, "for the edge bytes and the records", at.bytes, &tail)) return rc;
            HIP_TRY(h, hipMemsetAsync(tail + at.zero_from, 0, at.bytes - at.zero_from, f.stream));
            return graph_edge_walk(f, cut, n, in<uint32_t>(tail, at.edge_words), cols[0].at, cols[1].at, cols[2].at, nullptr);
        },
        [&](uint64_t n) -> int {
            const uint32_t *edge_words = in<uint32_t>(tail, at.edge_words);
            if (degrees) {
                uint64_t *d_table = in<uint64_t>(tail, at.table);
                HIP_TRY(h, launch_graph_degrees(edge_words, n, d_table, f.stream));
                HIP_TRY(h, hipMemcpyAsync(table, d_table, kGraphTableWords * 8, hipMemcpyDeviceToHost, f.stream));
                if (int rc = status_of(h, f.stream, f.which)) return rc;  // synchronises
                uint64_t edges = 0;
                for (uint32_t i = 0; i < kGraphTableWords; ++i) edges += uint64_t(i / kGraphDegrees) * table[i];  // (the in-degrees; the out-degrees sum to the same)
                if (out_edge_count) *out_edge_count = edges;
                return MSBWT_OK;
            }
            if (out_edges) HIP_TRY(h, hipMemcpyAsync(out_edges, edge_words, n, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, f.stream));
            if (!host) HIP_TRY(h, hipStreamSynchronize(f.stream));  // (the last chunk's edge pass, and the scratch is freed on return)
            return copy_out(f, cols, n);
        });
}

// ---- unitigs ----

// the walks of either call; its nodes (unitig_node_layout, canonical_unitig_layout) and outputs (unitig_output_layout) come on top
constexpr Shape kUnitigShape{true, false, 0, 0};
constexpr Shape kCanonicalUnitigShape{false, true, kCanonicalTotalWords * 8 < 256 ? 256 : kCanonicalTotalWords * 8, 0};  // (fixed: the walk's totals)
static_assert(MSBWT_UNITIG_INFO_WORDS == 8 && MSBWT_CANONICAL_UNITIG_INFO_WORDS == 10, "the header's constants");

// a msbwt_[canonical_]unitigs_plan: the walks of `p`, `node_bytes` over `nodes` nodes or classes and, unless it is the counting call
// (unitigs = symbols = 0), the outputs with all four columns staged
int unitigs_plan(const Shape &p, uint64_t node_bytes, uint64_t total_rows, uint64_t free_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t *device_bytes) {
    if (unitigs >= kMaxSymbols || symbols / 33 >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;  // (S <= 32 n + n)
    const uint64_t out = unitigs || symbols ? unitig_output_layout(unitigs, symbols, true, true, true, true).bytes : 0;
    return plan(p, total_rows, free_bytes, nodes, node_bytes + out, device_bytes);
}

// a msbwt_[canonical_]unitig_graph_plan: that plan and, unless it is the counting call (unitigs = symbols = links = 0), the link table
// with its targets staged
int unitig_graph_plan(const Shape &p, uint64_t node_bytes, uint64_t total_rows, uint64_t free_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links,
                      uint64_t *device_bytes) {
    if (links / 8 >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;  // (L <= 8 U)
    const bool fills = unitigs || symbols || links;
    const uint64_t out = fills ? unitig_output_layout(unitigs, symbols, true, true, true, true).bytes + unitig_link_layout(unitigs, links, true).bytes : 0;
    if (unitigs >= kMaxSymbols || symbols / 33 >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    return plan(p, total_rows, free_bytes, nodes, node_bytes + out, device_bytes);
}

// a msbwt_[canonical_]unitig_graph_by_source_plan: that plan and, unless it is the counting call, the block by source with the
// matrix of `n_sources` columns staged
int unitig_graph_by_source_plan(bool canonical, uint64_t total_rows, uint64_t free_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links, size_t n_sources,
                                uint64_t *device_bytes) {
    if (n_sources < 1 || n_sources > kSourceMax) return MSBWT_ERR_INVALID_ARG;
    uint64_t graph = 0;
    const uint64_t node_bytes = canonical ? canonical_unitig_layout(nodes).bytes : unitig_node_layout(nodes).bytes;
    if (int rc = unitig_graph_plan(canonical ? kCanonicalUnitigShape : kUnitigShape, node_bytes, total_rows, free_bytes, nodes, unitigs, symbols, links, &graph)) return rc;
    const bool fills = unitigs || symbols || links;
    if (device_bytes) *device_bytes = graph + (fills ? unitig_source_layout(unitig_source_range_words(nodes, canonical), unitigs, n_sources, true).bytes : 0);
    return MSBWT_OK;
}

uint64_t ceil_log2(uint64_t x) {
    uint64_t r = 0;
    while (r < 63 && (1ull << r) < x) ++r;
    return r;
}

// a kernel's counters on the host (synchronises)
template <size_t N>
int read_counters(Frame &f, const unsigned long long *d_counters, uint64_t (&c)[N]) {
    HIP_TRY(f.h, hipMemcpyAsync(c, d_counters, sizeof c, hipMemcpyDeviceToHost, f.stream));
    HIP_TRY(f.h, hipStreamSynchronize(f.stream));
    return MSBWT_OK;
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

// The outputs of a unitig call, plain or canonical.  open(): the frame's guard ladder with the call's own checks (args) and the
// thresholds' in it, then zeros in *out_unitigs, *out_symbol_total and the handle's info words.  emit(), once U and S are known:
// *out_unitigs and *out_symbol_total, the capacity contract, the second allocation (unitig_output_layout: the offsets, and the other
// four columns where a host form stages them), numbering and emission (skip_marked: heads carry kUnitigSkip).  deliver(): the copies.
// With `links` (the unitig graph calls) the link table rides along: open() zeroes *out_links too; emit() counts L before it looks at
// the capacities -- so that a capacity_links below L also writes nothing --, takes unitig_link_layout as a third allocation and
// runs degrees, scan and targets behind the emission (unitig_links.hpp); deliver() copies the offsets and the staged targets.
struct UnitigLinkOutputs {
    void *offsets, *targets;  // the caller's: 2 U + 1 words and L words, each may be nullptr
    uint64_t capacity;
    uint64_t *out_links;  // may be nullptr
    bool canonical;
    uint64_t expect = ~0ull;  // what the counters say L is, where they say it (the plain call)
    uint64_t L = 0;
    uint64_t *d_offsets = nullptr, *d_targets = nullptr;
};

// With `by_source` (the unitig graph calls by source) the U x S matrix rides along behind the links: open() asks for the attachment;
// a call that fills buffers and wants the matrix takes unitig_source_layout -- the plain call its range words before the edge walk,
// which leaves every node's l there; the rest in emit(), as one more allocation behind the link block -- and runs the sums behind the
// emission (unitig_sources.hpp), the canonical call a chunk of slots at a time behind a search for their ranges; deliver() copies it.
struct UnitigSourceOutputs {
    void *sums;  // the caller's: U x S words, may be nullptr
    bool canonical;
    uint64_t *l = nullptr;       // plain: every node's range start, n words
    uint64_t *chunk = nullptr;   // canonical: 32 bytes a slot of a chunk (the call's own, free behind the fold) ...
    uint64_t chunk_slots = 0;    // ... and the slots of a chunk
    uint64_t sources = 0;
    uint64_t *d_sums = nullptr;
};

struct UnitigOutputs {
    void *symbols, *offsets, *sums, *ends, *flags;
    uint64_t capacity_unitigs, capacity_symbols;
    uint64_t *out_unitigs, *out_symbol_total;
    UnitigLinkOutputs *links = nullptr;
    UnitigSourceOutputs *by_source = nullptr;
    uint64_t U = 0, S = 0;
    bool filled = false;
    uint64_t *d_offsets = nullptr, *d_sums = nullptr;
    uint8_t *d_symbols = nullptr, *d_ends = nullptr, *d_flags = nullptr;

    template <size_t W, class Args>
    int open(Frame &f, const GraphCut &cut, uint64_t (msbwt_rle::*info)[W], Args &&args) const {
        const auto checks = [&] { const int rc = args(); return rc ? rc : cut.check(f, out_unitigs); };
        if (int rc = f.open(by_source != nullptr, checks)) return rc;
        *out_unitigs = 0;
        if (out_symbol_total) *out_symbol_total = 0;
        if (links && links->out_links) *links->out_links = 0;
        std::fill(f.h->*info, f.h->*info + W, 0ull);
        return MSBWT_OK;
    }

    // the matrix is wanted, and the call fills buffers
    bool colours() const { return by_source && by_source->sums && (capacity_unitigs || capacity_symbols || (links && links->capacity)); }

    // the plain call's range words, before its edge walk: nullptr where the matrix is not wanted
    int take_ranges(Frame &f, uint64_t n, uint64_t **l) const {
        *l = nullptr;
        if (!colours() || by_source->canonical) return MSBWT_OK;
        char *block = nullptr;
        if (int rc = f.take_more(&block, unitig_source_layout(unitig_source_range_words(n, false), 0, 0, false).bytes, "for the ranges of the nodes")) return rc;
        *l = by_source->l = in<uint64_t>(block, 0);
        return MSBWT_OK;
    }

    int emit(Frame &f, const UnitigNodes &g, const UnitigState *state, UnitigState *heads, void *tiles, uint64_t unitigs, uint64_t total, bool skip_marked) {
        msbwt_rle *h = f.h;
        const bool host = f.host;
        U = unitigs;
        S = total;
        *out_unitigs = U;
        if (out_symbol_total) *out_symbol_total = S;
        if (links) {  // L, before anything is written: the tails' degrees added up
            uint64_t c[kUnitigLinkEntries + 1] = {};
            HIP_TRY(h, launch_unitig_link_degrees(g, state, nullptr, uint32_t(f.k), links->canonical, U, nullptr, nullptr, f.stream));
            if (int rc = read_counters(f, g.counters, c)) return rc;
            links->L = c[kUnitigLinkEntries];
            if (links->L > 8 * U || (links->expect != ~0ull && links->L != links->expect))
                return fail(h, MSBWT_ERR_INTERNAL, f.name + ": the sides hold " + std::to_string(links->L) + " entries, which the graph's counters do not bear out");
            if (links->out_links) *links->out_links = links->L;
        }
        if (capacity_unitigs == 0 && capacity_symbols == 0 && (!links || links->capacity == 0)) return MSBWT_OK;
        const std::string need = "U = " + std::to_string(U) + " unitigs of S = " + std::to_string(S) + " symbols";
        if (links && (capacity_unitigs < U || (symbols && capacity_symbols < S) || (links->targets && links->capacity < links->L)))
            return f.refuse(": the capacities " + std::to_string(capacity_unitigs) + ", " + std::to_string(capacity_symbols) + " and " + std::to_string(links->capacity) +
                            " are less than the " + need + " with L = " + std::to_string(links->L) + " links");
        if (capacity_unitigs < U || (symbols && capacity_symbols < S))
            return f.refuse(": the capacities " + std::to_string(capacity_unitigs) + " and " + std::to_string(capacity_symbols) + " are less than the " + need);
        const bool stage_sums = host && sums, stage_symbols = host && symbols, stage_ends = host && ends, stage_flags = host && flags;
        const UnitigOutputLayout at = unitig_output_layout(U, S, stage_sums, stage_symbols, stage_ends, stage_flags);
        char *block = nullptr, *link_block = nullptr;
        if (int rc = f.take_more(&block, at.bytes, "for the unitigs")) return rc;
        const UnitigLinkLayout link_at = links ? unitig_link_layout(U, links->L, host && links->targets) : UnitigLinkLayout{};
        if (links) {
            if (int rc = f.take_more(&link_block, link_at.bytes, "for the links")) return rc;
            links->d_offsets = in<uint64_t>(link_block, link_at.offsets);
            links->d_targets = host && links->targets ? in<uint64_t>(link_block, link_at.targets) : static_cast<uint64_t *>(links->targets);
        }
        uint64_t *pairs = nullptr;
        if (colours()) {
            UnitigSourceOutputs &bs = *by_source;
            bs.sources = h->sources.n_sources;
            const UnitigSourceLayout source_at = unitig_source_layout(bs.canonical ? 2 * bs.chunk_slots : 0, U, bs.sources, host);
            char *source_block = nullptr;
            if (source_at.bytes)
                if (int rc = f.take_more(&source_block, source_at.bytes, "for the sums by source")) return rc;
            if (bs.canonical) pairs = in<uint64_t>(source_block, source_at.ranges);
            bs.d_sums = host ? in<uint64_t>(source_block, source_at.sums) : static_cast<uint64_t *>(bs.sums);
        }
        // a device form's outputs are the caller's own; a staged one has its place in the block
        d_offsets = in<uint64_t>(block, at.offsets);
        d_sums = static_cast<uint64_t *>(stage_sums ? block + at.sums : sums);
        d_symbols = static_cast<uint8_t *>(stage_symbols ? block + at.symbols : symbols);
        d_ends = static_cast<uint8_t *>(stage_ends ? block + at.ends : ends);
        d_flags = static_cast<uint8_t *>(stage_flags ? block + at.flags : flags);
        if (d_sums) HIP_TRY(h, hipMemsetAsync(d_sums, 0, 8 * U, f.stream));
        HIP_TRY(h, launch_unitig_number(g, heads, tiles, uint32_t(f.k), U, S, d_offsets, f.stream));
        HIP_TRY(h, launch_unitig_emit(g, state, heads, uint32_t(f.k), U, S, d_symbols, d_sums, d_ends, d_flags, f.stream, skip_marked));
        if (links) {
            HIP_TRY(h, launch_unitig_link_degrees(g, state, heads, uint32_t(f.k), links->canonical, U, links->d_offsets, d_flags, f.stream));
            HIP_TRY(h, launch_unitig_link_scan(U, links->d_offsets, link_block + link_at.tiles, f.stream));
            if (links->d_targets)
                HIP_TRY(h, launch_unitig_link_targets(g, state, heads, uint32_t(f.k), links->canonical, uint32_t(ceil_log2(g.n) + 1), U, links->L, links->d_offsets,
                                                      links->d_targets, f.stream));
        }
        if (colours()) {
            const UnitigSourceOutputs &bs = *by_source;
            const SourceView view = h->sources.view(h->totals.total);
            const uint32_t probes = uint32_t(ceil_log2(g.n) + 1);
            HIP_TRY(h, hipMemsetAsync(bs.d_sums, 0, 8 * U * bs.sources, f.stream));
            if (!bs.canonical) {
                HIP_TRY(h, launch_unitig_source_sums(g, state, heads, uint32_t(f.k), false, probes, U, view, UnitigSourceRanges{bs.l, nullptr, 0, g.n}, bs.d_sums, f.stream));
            } else {
                // the slots hold words and class counts: a chunk's words as symbol bytes, their ranges by the library's search, the sums
                uint8_t *rows = reinterpret_cast<uint8_t *>(bs.chunk);
                for (uint64_t first = 0; first < g.n; first += bs.chunk_slots) {
                    const uint64_t m = std::min(bs.chunk_slots, g.n - first);
                    HIP_TRY(h, launch_unpack_rows(g.kmers + first, uint32_t(f.k), m, rows, f.stream));
                    if (int rc = timed_with_tickets(h, f.stream, [&](const IndexView &v) {
                            return launch_kmer_ranges(v, rows, uint32_t(f.k), m, pairs, pairs + 1, 2u, h->d_flags + f.which, f.stream);
                        }))
                        return rc;
                    HIP_TRY(h, launch_unitig_source_sums(g, state, heads, uint32_t(f.k), true, probes, U, view, UnitigSourceRanges{nullptr, pairs, first, m}, bs.d_sums, f.stream));
                }
            }
        }
        filled = true;
        return MSBWT_OK;
    }

    // a graph call that had capacities and found nothing to fill (an empty index, no node that counts): side 0 of no unitig starts at 0
    int close(Frame &f, int rc) const {
        if (rc || filled || !links || !links->offsets || !(capacity_unitigs || capacity_symbols || links->capacity)) return rc;
        if (f.host) {
            *static_cast<uint64_t *>(links->offsets) = 0;
            return MSBWT_OK;
        }
        HIP_TRY(f.h, hipMemsetAsync(links->offsets, 0, 8, f.stream));
        HIP_TRY(f.h, hipStreamSynchronize(f.stream));
        return MSBWT_OK;
    }

    int deliver(Frame &f) {
        msbwt_rle *h = f.h;
        if (filled) {
            const hipMemcpyKind kind = f.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
            if (offsets) HIP_TRY(h, hipMemcpyAsync(offsets, d_offsets, 8 * (U + 1), kind, f.stream));
            if (f.host && sums) HIP_TRY(h, hipMemcpyAsync(sums, d_sums, 8 * U, kind, f.stream));
            if (f.host && symbols) HIP_TRY(h, hipMemcpyAsync(symbols, d_symbols, S, kind, f.stream));
            if (f.host && ends) HIP_TRY(h, hipMemcpyAsync(ends, d_ends, U, kind, f.stream));
            if (f.host && flags) HIP_TRY(h, hipMemcpyAsync(flags, d_flags, U, kind, f.stream));
            if (links && links->offsets) HIP_TRY(h, hipMemcpyAsync(links->offsets, links->d_offsets, 8 * unitig_link_sides(U), kind, f.stream));
            if (links && f.host && links->targets && links->L) HIP_TRY(h, hipMemcpyAsync(links->targets, links->d_targets, 8 * links->L, kind, f.stream));
            if (f.host && colours()) HIP_TRY(h, hipMemcpyAsync(by_source->sums, by_source->d_sums, 8 * U * by_source->sources, kind, f.stream));
        }
        if (f.host) return status_of(h, f.stream, f.which);  // synchronises
        HIP_TRY(h, hipStreamSynchronize(f.stream));           // (the scratch is freed on return)
        return MSBWT_OK;
    }
};

// Both forms: the sorted dump's counting walk, the staged walk with the edge pass behind it (into scratch: words, counts, edge bytes
// and predecessor slots), then links, ranking, cycles, numbering and emission over the slots (unitigs.hpp).
int unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, bool host, void *out_symbols, void *out_offsets, void *out_sums, void *out_ends,
            void *out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs, uint64_t *out_symbol_total, hipStream_t stream,
            UnitigLinkOutputs *links = nullptr, UnitigSourceOutputs *by_source = nullptr) {
    Frame f(bwt, by_source ? "enumerate_unitig_graph_by_source" : links ? "enumerate_unitig_graph" : "enumerate_unitigs", k, host, stream);
    const GraphCut cut(min_count, min_edge);
    UnitigOutputs out{out_symbols, out_offsets, out_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total, links, by_source};
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
            if (links) links->expect = 2 * (c[kUnitigEdges] - c[kUnitigLinks] + c[kUnitigCircular]);  // (every edge that is no link, and a closing link, from both its ends)
            return out.emit(f, g, cur, other, block + at.tiles, U, S, false);
        },
        [&](uint64_t) { return out.deliver(f); });
    return out.close(f, rc);
}

// ---- canonical unitigs ----

// Both forms: the canonical walk counts the classes and then appends them; both members of every class become nodes in word order;
// the (k+1)-mers out of every node are counted and folded into D's edge bytes; then the compaction of the plain call over the N
// slots, with the cuts behind the links and the choice between a unitig and its mirror behind the ranking (canonical_unitigs.hpp).
int canonical_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, bool host, void *out_symbols, void *out_offsets, void *out_sums,
                      void *out_ends, void *out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                      hipStream_t stream, UnitigLinkOutputs *links = nullptr, UnitigSourceOutputs *by_source = nullptr) {
    Frame f(bwt, by_source ? "enumerate_canonical_unitig_graph_by_source" : links ? "enumerate_canonical_unitig_graph" : "enumerate_canonical_unitigs", k, host, stream);
    const GraphCut cut(min_count, min_edge);
    UnitigOutputs out{out_symbols, out_offsets, out_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs, out_symbol_total, links, by_source};
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
            if (by_source) {
                by_source->chunk = chunk;
                by_source->chunk_slots = at.chunk_slots;
            }
            return out.emit(f, g, cur, other, block + at.tiles, U, S, true);
        },
        [&](uint64_t) { return out.deliver(f); });
    return out.close(f, rc);
}

// ---- traces ----

constexpr uint64_t kTracePiece = 1ull << 20;  // the automatic piece
constexpr uint64_t kTraceLimit = 1ull << 40;  // max_steps, and the symbols of all rows, stay below
static_assert(MSBWT_TRACE_INFO_WORDS == 8 && MSBWT_TRACE_RIGHT == kTraceRight && MSBWT_TRACE_LEFT == kTraceLeft && MSBWT_TRACE_UNIQUE == kTraceUnique &&
                  MSBWT_TRACE_UNITIG == kTraceUnitig && MSBWT_TRACE_GREEDY == kTraceGreedy && MSBWT_TRACE_DEAD_END == kTraceDeadEnd && MSBWT_TRACE_BRANCH == kTraceBranch &&
                  MSBWT_TRACE_MERGE == kTraceMerge && MSBWT_TRACE_RETURNED == kTraceReturned && MSBWT_TRACE_TARGET == kTraceTarget &&
                  MSBWT_TRACE_MAX_STEPS == kTraceMaxSteps && MSBWT_TRACE_NOT_A_NODE == kTraceNotANode,
              "the header's constants");

bool trace_mode_ok(int mode) { return mode == kTraceUnique || mode == kTraceUnitig || mode == kTraceGreedy; }
bool trace_too_large(uint64_t n, uint64_t max_steps) { return max_steps >= kTraceLimit || (max_steps && n > (kTraceLimit - 1) / max_steps); }
uint64_t trace_piece_walks(uint64_t n, uint64_t piece) { return std::min(n, piece ? piece : kTracePiece); }

// Both forms.  A piece of walks at a time: the seeds become states and round 0's queries; then, round by round, the packed search
// over the live walks' queries and the one kernel that reads its counts (trace.hpp), until the live count the host reads back is 0
// -- after max_steps + 1 rounds at the most.  A host form stages a piece's seeds, targets and outputs in the call's block.
int trace_kmers(const msbwt_rle *bwt, const void *seeds, const void *targets, size_t k, size_t n, uint64_t min_count, uint64_t min_edge, int mode, int direction,
                uint64_t max_steps, bool host, void *out_symbols, void *out_steps, void *out_stops, void *out_edge_sums, void *out_last, void *out_fans, hipStream_t stream) {
    Frame f(bwt, "trace_kmers", k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = f.open(false, [&]() -> int {
            if (k > 31) return f.refuse(" needs 1 <= k <= 31 (an edge is a packed (k+1)-mer)");
            if (cut.me < cut.m) return f.refuse(": min_edge is below the node threshold (0 = the node threshold)");
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
        std::copy(info, info + MSBWT_TRACE_INFO_WORDS, h->trace_info);
        return rc;
    };
    std::fill(h->trace_info, h->trace_info + MSBWT_TRACE_INFO_WORDS, 0ull);
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
    const uint32_t q = trace_queries_per_walk(mode);
    const TraceLayout at = trace_layout(P, max_steps, mode, targets != nullptr, host);
    char *block = nullptr;
    if (int rc = f.take(&block, at.bytes, f.needs(at.bytes, false, "while it runs"), true)) return rc;
    c.counters = in<unsigned long long>(block, at.counters);
    uint64_t *queries = in<uint64_t>(block, at.queries), *counts = in<uint64_t>(block, at.counts);
    const struct {
        const void *caller;
        uint64_t at, bytes;  // where a piece's lies in the block, and the bytes a walk
    } inputs[] = {{seeds, at.seeds, 8}, {targets, at.targets, 8}}, outputs[] = {{out_symbols, at.symbols, max_steps}, {out_steps, at.steps, 8},      {out_stops, at.stops, 1},
                                                                                {out_edge_sums, at.edge_sums, 8},     {out_last, at.last, 8},        {out_fans, at.fans, 1}};
    if (host) {  // the kernels write a piece's staged columns, wanted or not
        c.seeds = in<const uint64_t>(block, at.seeds);
        c.targets = targets ? in<const uint64_t>(block, at.targets) : nullptr;
        c.symbols = in<uint8_t>(block, at.symbols);
        c.steps = in<uint64_t>(block, at.steps);
        c.stops = in<uint8_t>(block, at.stops);
        c.edge_sums = in<uint64_t>(block, at.edge_sums);
        c.last = in<uint64_t>(block, at.last);
        c.fans = in<uint8_t>(block, at.fans);
    }
    for (uint64_t first = 0; first < n; first += P) {
        const uint64_t walks = std::min(P, n - first);
        if (host) {
            c.first = first;
            c.rows = walks;
            for (const auto &col : inputs)
                if (col.caller) HIP_TRY(h, hipMemcpyAsync(block + col.at, static_cast<const char *>(col.caller) + first * col.bytes, walks * col.bytes, hipMemcpyHostToDevice, f.stream));
            // a row's tail behind its symbols stays the caller's: the rows go up before they come down
            if (out_symbols && max_steps) HIP_TRY(h, hipMemcpyAsync(c.symbols, static_cast<const char *>(out_symbols) + first * max_steps, walks * max_steps, hipMemcpyHostToDevice, f.stream));
        }
        TraceWalk *cur = in<TraceWalk>(block, at.states[0]), *other = in<TraceWalk>(block, at.states[1]);
        HIP_TRY(h, hipMemsetAsync(c.counters, 0, kTraceCounterBytes, f.stream));
        HIP_TRY(h, launch_trace_seed(c, first, walks, cur, queries, f.stream));
        if (int rc = launch_count_2bit(h, queries, k, size_t(walks), counts, f.stream, f.which)) return rc;
        if (int rc = launch_count_2bit(h, queries + walks, k + 1, size_t(4 * walks), counts + walks, f.stream, f.which)) return rc;
        info[2] += 5 * walks;
        uint64_t live = walks, left[kTraceCounterWords] = {};
        for (uint64_t round = 0; live && round <= max_steps; ++round) {
            if (round) {
                if (int rc = launch_count_2bit(h, queries, k + 1, size_t(q * live), counts, f.stream, f.which)) return rc;
                info[2] += q * live;
            }
            HIP_TRY(h, hipMemsetAsync(c.counters + kTraceLive, 0, 8, f.stream));
            HIP_TRY(h, launch_trace_round(c, round == 0, walks, live, cur, counts, other, queries, f.stream));
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
            for (const auto &col : outputs)
                if (col.caller && col.bytes) HIP_TRY(h, hipMemcpyAsync(static_cast<char *>(const_cast<void *>(col.caller)) + first * col.bytes, block + col.at, walks * col.bytes, hipMemcpyDeviceToHost, f.stream));
    }
    if (host) return close(status_of(h, f.stream, f.which));  // synchronises
    HIP_TRY(h, hipStreamSynchronize(f.stream));                // (the scratch is freed on return)
    return close(MSBWT_OK);
}

// what a family's last call on the handle left in its info words
template <size_t W>
int info_words(const msbwt_rle *bwt, uint64_t (msbwt_rle::*info)[W], uint64_t *out) {
    Call c(bwt);
    if (!c.h || !out) return MSBWT_ERR_INVALID_ARG;
    std::copy(c.h->*info, c.h->*info + W, out);
    return MSBWT_OK;
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

// ---- the k-mer graph: an edge byte per k-mer of the sorted dump, and the table of (in, out) degrees ----

int msbwt_rle_enumerate_kmer_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_kmers2bit, uint64_t *out_counts, uint64_t *out_l,
                                   uint8_t *out_edges, uint64_t capacity, uint64_t *out_n) {
    return kmer_graph(bwt, k, min_count, min_edge, true, out_kmers2bit, out_counts, out_l, out_edges, capacity, out_n, nullptr, nullptr, nullptr);
}

int msbwt_rle_enumerate_kmer_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_kmers2bit, void *d_out_counts, void *d_out_l,
                                          void *d_out_edges, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return kmer_graph(bwt, k, min_count, min_edge, false, d_out_kmers2bit, d_out_counts, d_out_l, d_out_edges, capacity, out_n, nullptr, nullptr,
                      static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_kmer_graph_degrees(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_table, uint64_t *out_nodes, uint64_t *out_edges) {
    uint64_t unwanted[kGraphTableWords];
    return kmer_graph(bwt, k, min_count, min_edge, true, nullptr, nullptr, nullptr, nullptr, 0, out_nodes, out_table ? out_table : unwanted, out_edges, nullptr);
}

// the host dump of `records` nodes with words, counts and l
int msbwt_kmer_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes) {
    return plan(graph_shape(true), total_rows, free_hbm_bytes, records, graph_tail_layout(records).bytes - graph_tail_layout(0).bytes, device_bytes);
}

// ---- unitigs: the non-branching paths of the k-mer graph as ragged sequences ----

int msbwt_rle_enumerate_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets, uint64_t *out_count_sums,
                                uint8_t *out_ends, uint8_t *out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs,
                                uint64_t *out_symbol_total) {
    return unitigs(bwt, k, min_count, min_edge, true, out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs,
                   out_symbol_total, nullptr);
}

int msbwt_rle_enumerate_unitigs_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                       void *d_out_count_sums, void *d_out_ends, void *d_out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                       uint64_t *out_unitigs, uint64_t *out_symbol_total, void *hip_stream) {
    return unitigs(bwt, k, min_count, min_edge, false, d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols,
                   out_unitigs, out_symbol_total, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_unitig_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::unitig_info, out); }

// the host call of `nodes` nodes that fills every buffer with `unitigs` unitigs of `symbols` symbols (none of either: the counting call)
int msbwt_unitigs_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t *device_bytes) {
    return unitigs_plan(kUnitigShape, unitig_node_layout(nodes).bytes, total_rows, free_hbm_bytes, nodes, unitigs, symbols, device_bytes);
}

// ---- canonical unitigs: the non-branching paths of the strand-merged k-mer graph ----

int msbwt_rle_enumerate_canonical_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                          uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                          uint64_t *out_unitigs, uint64_t *out_symbol_total) {
    return canonical_unitigs(bwt, k, min_count, min_edge, true, out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols,
                             out_unitigs, out_symbol_total, nullptr);
}

int msbwt_rle_enumerate_canonical_unitigs_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                                 void *d_out_count_sums, void *d_out_ends, void *d_out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                                 uint64_t *out_unitigs, uint64_t *out_symbol_total, void *hip_stream) {
    return canonical_unitigs(bwt, k, min_count, min_edge, false, d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs,
                             capacity_symbols, out_unitigs, out_symbol_total, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_canonical_unitig_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::canonical_unitig_info, out); }

// ---- unitig graphs: either unitig call with the link table of the compacted graph behind it ----

int msbwt_rle_enumerate_unitig_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                     uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets, uint64_t *out_link_targets,
                                     uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                     uint64_t *out_links) {
    UnitigLinkOutputs links{out_link_offsets, out_link_targets, capacity_links, out_links, false};
    return unitigs(bwt, k, min_count, min_edge, true, out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs,
                   out_symbol_total, nullptr, &links);
}

int msbwt_rle_enumerate_unitig_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                            void *d_out_count_sums, void *d_out_ends, void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                            uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                            uint64_t *out_links, void *hip_stream) {
    UnitigLinkOutputs links{d_out_link_offsets, d_out_link_targets, capacity_links, out_links, false};
    return unitigs(bwt, k, min_count, min_edge, false, d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols,
                   out_unitigs, out_symbol_total, static_cast<hipStream_t>(hip_stream), &links);
}

int msbwt_rle_enumerate_canonical_unitig_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                               uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets, uint64_t *out_link_targets,
                                               uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs,
                                               uint64_t *out_symbol_total, uint64_t *out_links) {
    UnitigLinkOutputs links{out_link_offsets, out_link_targets, capacity_links, out_links, true};
    return canonical_unitigs(bwt, k, min_count, min_edge, true, out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols,
                             out_unitigs, out_symbol_total, nullptr, &links);
}

int msbwt_rle_enumerate_canonical_unitig_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                                      void *d_out_count_sums, void *d_out_ends, void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                                      uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs,
                                                      uint64_t *out_symbol_total, uint64_t *out_links, void *hip_stream) {
    UnitigLinkOutputs links{d_out_link_offsets, d_out_link_targets, capacity_links, out_links, true};
    return canonical_unitigs(bwt, k, min_count, min_edge, false, d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs,
                             capacity_symbols, out_unitigs, out_symbol_total, static_cast<hipStream_t>(hip_stream), &links);
}

// the host call that fills every buffer, the two link arrays included (none of unitigs, symbols and links: the counting call)
int msbwt_unitig_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links, uint64_t *device_bytes) {
    return unitig_graph_plan(kUnitigShape, unitig_node_layout(nodes).bytes, total_rows, free_hbm_bytes, nodes, unitigs, symbols, links, device_bytes);
}

int msbwt_canonical_unitig_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols, uint64_t links,
                                      uint64_t *device_bytes) {
    return unitig_graph_plan(kCanonicalUnitigShape, canonical_unitig_layout(classes).bytes, total_rows, free_hbm_bytes, classes, unitigs, symbols, links, device_bytes);
}

// ---- unitig graphs by source: either unitig graph call with the U x S matrix of per-input sums behind the link table ----

int msbwt_rle_enumerate_unitig_graph_by_source(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols, uint64_t *out_offsets,
                                               uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets, uint64_t *out_link_targets,
                                               uint64_t *out_source_sums, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                               uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links) {
    UnitigLinkOutputs links{out_link_offsets, out_link_targets, capacity_links, out_links, false};
    UnitigSourceOutputs by_source{out_source_sums, false};
    return unitigs(bwt, k, min_count, min_edge, true, out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols, out_unitigs,
                   out_symbol_total, nullptr, &links, &by_source);
}

int msbwt_rle_enumerate_unitig_graph_by_source_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols, void *d_out_offsets,
                                                      void *d_out_count_sums, void *d_out_ends, void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                                      void *d_out_source_sums, uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                                      uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links, void *hip_stream) {
    UnitigLinkOutputs links{d_out_link_offsets, d_out_link_targets, capacity_links, out_links, false};
    UnitigSourceOutputs by_source{d_out_source_sums, false};
    return unitigs(bwt, k, min_count, min_edge, false, d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs, capacity_symbols,
                   out_unitigs, out_symbol_total, static_cast<hipStream_t>(hip_stream), &links, &by_source);
}

int msbwt_rle_enumerate_canonical_unitig_graph_by_source(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols,
                                                         uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags,
                                                         uint64_t *out_link_offsets, uint64_t *out_link_targets, uint64_t *out_source_sums, uint64_t capacity_unitigs,
                                                         uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                                         uint64_t *out_links) {
    UnitigLinkOutputs links{out_link_offsets, out_link_targets, capacity_links, out_links, true};
    UnitigSourceOutputs by_source{out_source_sums, true};
    return canonical_unitigs(bwt, k, min_count, min_edge, true, out_symbols, out_offsets, out_count_sums, out_ends, out_flags, capacity_unitigs, capacity_symbols,
                             out_unitigs, out_symbol_total, nullptr, &links, &by_source);
}

int msbwt_rle_enumerate_canonical_unitig_graph_by_source_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols,
                                                                void *d_out_offsets, void *d_out_count_sums, void *d_out_ends, void *d_out_flags,
                                                                void *d_out_link_offsets, void *d_out_link_targets, void *d_out_source_sums, uint64_t capacity_unitigs,
                                                                uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                                                uint64_t *out_links, void *hip_stream) {
    UnitigLinkOutputs links{d_out_link_offsets, d_out_link_targets, capacity_links, out_links, true};
    UnitigSourceOutputs by_source{d_out_source_sums, true};
    return canonical_unitigs(bwt, k, min_count, min_edge, false, d_out_symbols, d_out_offsets, d_out_count_sums, d_out_ends, d_out_flags, capacity_unitigs,
                             capacity_symbols, out_unitigs, out_symbol_total, static_cast<hipStream_t>(hip_stream), &links, &by_source);
}

// the graph plan of the same kind and, unless it is the counting call, unitig_source_layout with the matrix staged
int msbwt_unitig_graph_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols, uint64_t links, size_t n_sources,
                                      uint64_t *device_bytes) {
    return unitig_graph_by_source_plan(false, total_rows, free_hbm_bytes, nodes, unitigs, symbols, links, n_sources, device_bytes);
}

int msbwt_canonical_unitig_graph_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols, uint64_t links,
                                                size_t n_sources, uint64_t *device_bytes) {
    return unitig_graph_by_source_plan(true, total_rows, free_hbm_bytes, classes, unitigs, symbols, links, n_sources, device_bytes);
}

// the host call over `classes` classes that fills every buffer with `unitigs` unitigs of `symbols` symbols (none of either: the counting call)
int msbwt_canonical_unitigs_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols, uint64_t *device_bytes) {
    return unitigs_plan(kCanonicalUnitigShape, canonical_unitig_layout(classes).bytes, total_rows, free_hbm_bytes, classes, unitigs, symbols, device_bytes);
}

int msbwt_rle_trace_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge, int mode,
                          int direction, uint64_t max_steps, uint8_t *out_symbols, uint64_t *out_steps, uint8_t *out_stops, uint64_t *out_edge_sums, uint64_t *out_last,
                          uint8_t *out_fans) {
    return trace_kmers(bwt, seeds2bit, targets2bit, k, n, min_count, min_edge, mode, direction, max_steps, true, out_symbols, out_steps, out_stops, out_edge_sums, out_last,
                       out_fans, nullptr);
}

int msbwt_rle_trace_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit, size_t k, size_t n, uint64_t min_count, uint64_t min_edge,
                                 int mode, int direction, uint64_t max_steps, void *d_out_symbols, void *d_out_steps, void *d_out_stops, void *d_out_edge_sums,
                                 void *d_out_last, void *d_out_fans, void *hip_stream) {
    return trace_kmers(bwt, d_seeds2bit, d_targets2bit, k, n, min_count, min_edge, mode, direction, max_steps, false, d_out_symbols, d_out_steps, d_out_stops,
                       d_out_edge_sums, d_out_last, d_out_fans, static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_trace_info(const msbwt_rle *bwt, uint64_t *out) { return info_words(bwt, &msbwt_rle::trace_info, out); }

int msbwt_rle_set_trace_piece(msbwt_rle *bwt, uint64_t walks) {
    if (!bwt) return MSBWT_ERR_INVALID_ARG;
    return set_locked(bwt, bwt->trace_piece, walks);
}

// the one block of a call on an index that holds something: trace_layout at the piece the call takes
int msbwt_trace_plan(uint64_t n, uint64_t max_steps, int mode, int targets, int host, uint64_t piece, uint64_t *device_bytes) {
    if (!trace_mode_ok(mode)) return MSBWT_ERR_INVALID_ARG;
    if (trace_too_large(n, max_steps)) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) *device_bytes = n ? trace_layout(trace_piece_walks(n, piece), max_steps, mode, targets != 0, host != 0).bytes : 0;
    return MSBWT_OK;
}

}  // extern "C"
