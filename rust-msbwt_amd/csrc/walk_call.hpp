// What the k-mer walk calls of a loaded index share (spectrum.cpp, graph_calls.cpp, unitig_calls.cpp, trace_calls.cpp; included by those
// only): the host side of a call, written once.  The names live in msbwt_capi, as handle.hpp's do; the functions that are no templates
// are defined in walk_call.cpp.
//   Frame         a call: the locked handle, the guard ladder (no index, no sources, k, the call's own arguments, the device), the
//                 stream, the clock, the SpectrumInfo and the scratch -- allocated per call, freed before it returns -- and, built from
//                 the one name the call passes, every text it can say
//   Shape         what a family allocates: its msbwt_*_plan and the sufficiency check of take_scratch are the same sum over it
//   Column        an output array of a call: the caller's, and where the kernels write it -- stage_records carves a dump's from one
//                 allocation, place() puts a table's where its layout (graph_layouts.hpp) says; copy_columns / copy_out hand them over
//   two_pass      a dump: the counting pass, *out_n, the capacity pattern, the filling pass, the record after either
//   staged_walk   a walk whose chunks go to a sink behind it; canonical_walk: the one with the other strand counted by the packed search
//   GraphCut / count_nodes / graph_edge_walk   the thresholds of the graph, unitig and trace calls, the sorted dump's counting walk and
//                 the staged walk with the edge pass behind it
//   in / read_counters / ceil_log2 / info_words   an array of a block, a kernel's counters on the host, and a family's info getter
// A unit's body is what is left: its argument checks, its sink, and the order of its passes.
#pragma once
#include <algorithm>
#include <chrono>
#include <string>

#include "handle.hpp"
#include "run_encode.hpp"
#include "spectrum.hpp"

namespace msbwt {
struct CanonicalSink;  // canonical.hpp
}

namespace msbwt_capi __attribute__((visibility("hidden"))) {

constexpr uint64_t kRecordBytes = 3 * sizeof(uint64_t);  // of a dump: k-mer, count, l

// ---- what a family allocates ----

// The scratch of a call beyond the walk's own frontiers.  A plan counts `record_bytes` per record staged for a host dump; the call
// itself stages only the columns its caller wants.
struct Shape {
    bool rank;              // the bitmap over the rows and its checkpoints: a sorted call that fills buffers
    bool canonical;         // kCanonicalStageBytes per frontier node: the other strand of a chunk's k-mers
    uint64_t fixed;         // the sink's words, the histograms
    uint64_t record_bytes;
};

uint64_t shape_bytes(const Shape &p, uint64_t total_rows, uint64_t frontier, uint64_t records);
// a msbwt_*_plan: the shape at the automatic frontier, and `more`; MSBWT_ERR_TOO_LARGE for what no index can be
int plan(const Shape &p, uint64_t total_rows, uint64_t free_bytes, uint64_t records, uint64_t more, uint64_t *device_bytes);

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
    void record();
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
SpectrumSeeds seeds_of(const Frame &f);

// The frontiers and what else of `p` does not wait for the records (the rank scratch, the canonical staging and totals) in HBM, or
// MSBWT_ERR_HIP naming the bytes of the shape.  p.fixed is checked for here and taken by the call.
int take_scratch(Frame &f, const Shape &p);

// ---- the output arrays of a call ----

// A column: the caller's array (`out`: of the host or of the device, as the frame says; nullptr = not wanted) of `rows` rows of `bytes`
// bytes, and where the kernels write it (`at`).  A dump's columns share their rows and lie where stage_records puts them; a table's say
// where their layout has them in the call's block (`offset`), and one that is `scratch` lies there in either form, wanted or not --
// the kernels write it anyway -- and is copied with the frame's kind.
struct Column {
    void *out = nullptr;
    uint64_t bytes = 8;
    uint64_t rows = 0;
    uint64_t offset = 0;
    bool scratch = false;
    void *at = nullptr;
    template <class T>
    T *as() const {
        return static_cast<T *>(at);
    }
};

// Where the sink of a dump writes: a device form's columns are the caller's own; a host form's are carved from one allocation of the n
// records' wanted bytes -- *capacity becomes n --, `tail_bytes` more behind them in either form (*tail).  Nothing to stage and no tail: no allocation.
template <size_t N>
int stage_records(Frame &f, Column (&cols)[N], uint64_t n, uint64_t *capacity, const char *for_what, uint64_t tail_bytes = 0, char **tail = nullptr) {
    uint64_t row = 0;
    for (Column &c : cols) {
        c.at = c.out;
        c.rows = n;
        if (f.host && c.out) row += c.bytes;
    }
    const uint64_t bytes = n * row + tail_bytes;
    if (bytes == 0) return MSBWT_OK;
    char *block = nullptr;
    if (int rc = f.take_more(&block, bytes, for_what)) return rc;
    if (tail) *tail = block + n * row;
    if (!f.host) return MSBWT_OK;
    for (Column &c : cols)
        if (c.out) {
            c.at = block;
            block += n * c.bytes;
        }
    *capacity = n;
    return MSBWT_OK;
}

// Where the kernels write a table: a scratch column and a host form's wanted one at their offsets in `block`, a device form's in the
// caller's own array (nullptr: not wanted).
template <size_t N>
void place(const Frame &f, Column (&cols)[N], char *block) {
    for (Column &c : cols) c.at = c.scratch || (f.host && c.out) ? block + c.offset : c.out;
}

// The wanted columns that do not lie in the caller's arrays already, copied there: a host form's, and the scratch ones of either form.
template <size_t N>
int copy_columns(Frame &f, const Column (&cols)[N]) {
    const hipMemcpyKind kind = f.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    for (const Column &c : cols)
        if (c.out && c.rows && (f.host || c.scratch)) HIP_TRY(f.h, hipMemcpyAsync(c.out, c.at, c.rows * c.bytes, kind, f.stream));
    return MSBWT_OK;
}

// A host form's wanted columns copied out, and the flags its kernels left (synchronises).  A device form has its records where they
// belong, and a fault is in the device status word: msbwt_rle_device_status.
template <size_t N>
int copy_out(Frame &f, const Column (&cols)[N]) {
    if (!f.host) return MSBWT_OK;
    if (int rc = copy_columns(f, cols)) return rc;
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
int staged_walk(Frame &f, uint64_t prune, unsigned long long *d_totals, uint32_t words, uint64_t *totals, const SpectrumChunkHook &per_chunk);

// One walk of a canonical call: the reverse complements of a chunk's k-mers are written as packed words and counted by the packed
// search, and the classes they emit go to `sink` (its totals: f.totals, copied to totals[] at the end).  Synchronises the stream.
int canonical_walk(Frame &f, uint64_t prune, CanonicalSink sink, uint64_t *totals);

// ---- the k-mer graph under the graph, unitig and trace calls ----

// What they take for a node and for an edge: a k-mer at least m wide, a (k+1)-mer at least me.
struct GraphCut {
    uint64_t m, me;
    GraphCut(uint64_t min_count, uint64_t min_edge) : m(std::max<uint64_t>(min_count, 1)), me(min_edge ? min_edge : m) {}
    int thresholds(const Frame &f) const { return me < m ? f.refuse(": min_edge is below the node threshold (0 = the node threshold)") : int(MSBWT_OK); }
    // a graph or unitig call's own rung of the guard ladder: the thresholds, then the output no call can do without
    int check(const Frame &f, const void *needed) const {
        if (int rc = thresholds(f)) return rc;
        return !needed ? fail(f.h, MSBWT_ERR_INVALID_ARG, "null pointer") : int(MSBWT_OK);
    }
};

// the sorted dump's counting walk: the scratch of `p`, *n = the nodes, and with p.rank the bit of every node's l
int count_nodes(Frame &f, const Shape &p, const GraphCut &cut, uint64_t *n);

// The staged walk with the edge pass behind it: the n nodes' columns (each optional) at the rank of their l, their edge bytes ORed into
// edge_words (zeroed by the caller) and, where pred is given, the slot of a predecessor.
int graph_edge_walk(Frame &f, const GraphCut &cut, uint64_t n, uint32_t *edge_words, uint64_t *kmers, uint64_t *counts, uint64_t *l, uint64_t *pred);

// ---- small things ----

// an array of a block, at the offset its layout gives (graph_layouts.hpp)
template <class T>
T *in(char *block, uint64_t offset) {
    return reinterpret_cast<T *>(block + offset);
}

// a kernel's counters on the host (synchronises)
template <size_t N>
int read_counters(Frame &f, const unsigned long long *d_counters, uint64_t (&c)[N]) {
    HIP_TRY(f.h, hipMemcpyAsync(c, d_counters, sizeof c, hipMemcpyDeviceToHost, f.stream));
    HIP_TRY(f.h, hipStreamSynchronize(f.stream));
    return MSBWT_OK;
}

uint64_t ceil_log2(uint64_t x);

// what a family's last call on the handle left in its info words
template <size_t W>
int info_words(const msbwt_rle *bwt, uint64_t (msbwt_rle::*info)[W], uint64_t *out) {
    Call c(bwt);
    if (!c.h || !out) return MSBWT_ERR_INVALID_ARG;
    std::copy(c.h->*info, c.h->*info + W, out);
    return MSBWT_OK;
}

}  // namespace msbwt_capi
