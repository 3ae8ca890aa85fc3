// What the units of the C API share (capi.cpp, index_build.cpp, query.cpp, sources.cpp, produce.cpp, multi_device.cpp; included by those only): the handle,
// the parts of its index, its status block's layout and the plumbing of a call.  Shared names live in msbwt_capi, hidden from the library's
// symbol table; a unit's own names stay in its anonymous namespace.  The helpers declared here are defined in capi.cpp, launch_count and launch_count_2bit in query.cpp, attach_sources in sources.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "../../include/msbwt_hip.h"
#include "host_pipeline.hpp"
#include "kernels.hpp"
#include "merge.hpp"
#include "plane_index.hpp"
#include "reads_build.hpp"
#include "rle_codec.hpp"
#include "sparse_build.hpp"
#include "source_index.hpp"
#include "sparse_policy.hpp"
#include "table_policy.hpp"

using namespace msbwt;

namespace msbwt_capi __attribute__((visibility("hidden"))) {

// The parts of a loaded index beyond its blocks own their device buffers: release() frees them and resets the part.
// Direct table (kernels.hpp, TableView) of the index in HBM, with the side array of its escape lines and the presence filter made from it
struct DirectTable {
    void *entries = nullptr;
    int depth = 0;               // symbols a table entry stands for
    bool packed = false;         // packed lines (two levels deeper than the flat table it was made from)
    size_t bytes = 0;
    void *side = nullptr;        // packed table: flat entries of its escape lines (512 bytes per line), or nullptr
    uint64_t side_bytes = 0;
    uint64_t lines = 0, escape_lines = 0;  // of the packed table
    uint32_t *filter = nullptr;  // presence bits over the low 2*filter_depth index bits of the table
    int filter_depth = 0;
    void release_filter() {
        if (filter) (void)hipFree(filter);
        filter = nullptr;
        filter_depth = 0;
    }
    void release() {
        if (entries) (void)hipFree(entries);
        if (side) (void)hipFree(side);
        release_filter();
        *this = DirectTable{};
    }
    TableView view() const {  // (without a table: the filter depth alone)
        return entries ? TableView{entries, depth, packed, filter, filter_depth, packed ? side : nullptr} : TableView{nullptr, 0, false, nullptr, filter_depth};
    }
};

// One level of the sparse suffix table (sparse_table.hpp): ranges of the suffixes that occur, deeper than the direct table reaches
struct SparseLevel {
    void *lines = nullptr;       // (nbuckets + probe) lines of 128 bytes
    void *side = nullptr;        // 16-byte {l, h} entries of its ESCAPE entries
    uint64_t bytes = 0, side_bytes = 0, entries = 0;  // (entries: the second level's; the first level's are in the handle's sparse_report)
    uint32_t nbuckets = 0, probe = 0;
    int depth = 0;
    bool tier = false;           // of the two-tier form (entries for the suffixes at least 2 wide, filter bits for the rest)
    void release() {
        if (lines) (void)hipFree(lines);
        if (side) (void)hipFree(side);
        *this = SparseLevel{};
    }
    SparseView view() const { return lines ? SparseView{lines, nbuckets, uint32_t(depth), probe, side, tier ? 1u : 0u} : SparseView{}; }
};

// Pair index (two symbols per step, rank_ops.hpp)
struct PairIndex {
    void *blocks = nullptr;
    void *super = nullptr;
    uint64_t bytes = 0;
    uint64_t overlap_bytes = 0;  // what overlapping pair blocks take beyond disjoint ones (0 unless the data-driven policy chose them)
    int stride = 128;            // spacing of the pair blocks in HBM: 128, or 96 (overlapping); read only beside pair blocks
    void release() {  // (the stride stays: it describes the last pair index built)
        if (blocks) (void)hipFree(blocks);
        if (super) (void)hipFree(super);
        blocks = super = nullptr;
        bytes = overlap_bytes = 0;
    }
};

// Source colouring of a merged index (source_index.hpp): the input every row came from and the checkpoints over it.  Attached by
// msbwt_rle_set_sources / msbwt_rle_load_merged_many_sources (sources.cpp), dropped with the index; attached <=> n_sources != 0.
struct SourceIndex {
    void *rows = nullptr;
    void *checkpoints = nullptr;
    uint32_t n_sources = 0;
    uint64_t bytes = 0;               // of both arrays: msbwt_source_index_plan
    uint64_t totals[kSourceMax] = {};  // rows per source
    void release() {
        if (rows) (void)hipFree(rows);
        if (checkpoints) (void)hipFree(checkpoints);
        *this = SourceIndex{};
    }
    SourceView view(uint64_t total) const {
        return SourceView{static_cast<const uint8_t *>(rows), static_cast<const uint64_t *>(checkpoints), total, n_sources, source_stride(n_sources)};
    }
};

// What the caller has asked for: the settings the index is built by.  A replica copies them whole (msbwt_rle_replicate).
struct Settings {
    int wanted_block_format = kBlocksPlanes;  // takes effect at the next load
    int wanted_pair = -1;           // -1 = on when it fits comfortably, 0 = off, 1 = on
    int wanted_pair_stride = 0;     // 0 = automatic (table_policy.hpp: cheap -> 96; else 96 when the data keep ranges wide and it fits)
    int wanted_table_side = 1;      // 0 = no side array (queries of escape lines search from scratch, as until round 3)
    int wanted_second = -1;         // second sparse level: -1 = automatic (k undeclared, the deep direct table does not fit, this one does), 0 = never
    int wanted_tiers = -1;          // -1 = two-tier where the complete table of a depth does not fit, 0 = complete tables only, 1 = two-tier only
    int wanted_streaming = -1;      // index lines fetched non-temporally: -1 = when the random-access arrays dwarf the caches, 0 = never, 1 = always
    int wanted_sparse = -1;         // -1 = automatic (beside a pair index, as deep as the data and HBM allow, at most 23 -- or what query_length says), 0 = off, 16..28 = that depth
    int query_length = 0;           // the k the index will mostly be asked about (msbwt_rle_set_query_length), 0 = unknown
    int wanted_table_packed = -1;   // -1 = pack when the data warrants it and it fits, 0 = never, 1 = whenever a pair index exists
    int wanted_filter = -1;         // -1 = keep it when it can reject something, 0 = off
    int wanted_table_depth = -1;    // -1 = pick from the index size
    int search_kernel = kSearchAuto;
    int wanted_order = -1;          // batch order: 1 = whenever the passes apply; 0 and -1 (automatic: see order_pays) = never
    int order_bits = 22;            // key bits the bucket passes order by (11 in the global pass + 11 inside each bucket)
    uint64_t build_piece = 0;       // most suffixes the builder from reads sorts at once (0 = automatic, from the free HBM)
    uint64_t memory_budget = 0;     // bytes of HBM the index may hold (0 = no budget): msbwt_rle_set_memory_budget
    bool planned = false;           // a budget is in force: `plan` (table_policy.hpp, plan_index) decides the optional structures
    IndexPlan plan{};
};

}  // namespace msbwt_capi

using namespace msbwt_capi;

struct msbwt_rle : Settings {
    int device = 0;
    uint8_t bin_power = 8;
    bool loaded = false;
    Totals totals{};
    void *d_blocks = nullptr;
    uint64_t nblocks = 0;
    int block_format = kBlocksPlanes;         // format of d_blocks
    void *d_overflow = nullptr;               // run blocks: plane-shaped lines of the overflowing blocks
    uint64_t overflow_bytes = 0;
    PairIndex pair;                 // optional
    double typical_width = -1.0;    // median occurrence count of a present 24-mer, probed at load time (-1: not probed)
    DirectTable table;
    // sparse suffix table: `sparse`, and a second, shallower level (round 6; k undeclared) that serves the queries shorter than the first
    // one's entries (17 <= k < 23), which would otherwise fall to the direct table -- shallow beside a sparse table -- and lose 1.5-2.5 x
    // against the index without one
    SparseLevel sparse, sparse2;
    SparseBuildReport sparse_report{};
    SourceIndex sources;             // optional, the caller's explicit request: outside the memory budget's plan
    bool counting = false;           // search counters wanted (msbwt_rle_set_search_counters)
    // Tile-ticket counter blocks of the lanes kernel (kernels.hpp, kTicketBytes each): a launch takes a block whose
    // previous launch has COMPLETED (its event says so) or a new one, so two launches in flight on different
    // streams never share counters however many there are.
    struct TicketSlot {
        void *counters = nullptr;
        hipEvent_t done = nullptr;
        bool used = false;  // `done` has been recorded at least once
        hipStream_t last_stream = nullptr;  // the stream of the launch that used it last
        void *order_scratch = nullptr;      // scratch of the batch-ordering pass (order.hip) of the launch that holds the slot
        size_t order_bytes = 0;
        void *range_scratch = nullptr;      // the dense {l, h} pairs between the two phases of a by-source count (grow-only, as order_scratch)
        size_t range_bytes = 0;
    };
    std::vector<TicketSlot> tickets;
    // device status block (128 bytes): word 0 = flags of the host-pointer entry points (handle
    // stream), word 1 = flags of the *_device entry points (caller streams; read and cleared only by
    // msbwt_rle_device_status), bytes 64.. = 8 x u64 record of a failed device consistency check
    uint32_t *d_flags = nullptr;
    hipStream_t stream = nullptr;  // used by the host-pointer entry points
    void *d_stage = nullptr;
    size_t stage_bytes = 0;
    HostPipeline pipe;             // pinned, triple-buffered path of the host-pointer batch entry points
    // Small host batches (the trait's single-query calls above all): queries and results travel through ONE
    // mapped, coherent host buffer that the kernel reads and writes directly -- no copies, no memset, no flag
    // read-back; one launch and one stream synchronisation per call.
    void *d_gather = nullptr;      // scratch of msbwt_rle_allgather_counts (narrow wire widths)
    size_t gather_bytes = 0;
    hipStream_t gather_stream = nullptr;  // msbwt_rle_count_kmers_allgather_device: the all-gathers of a batch's pieces run here, beside the search
    std::vector<hipEvent_t> piece_events;
    uint8_t *mail = nullptr;       // host address
    uint8_t *d_mail = nullptr;     // the same buffer as the device sees it
    uint64_t mail_seq = 0;         // completion word of the mailbox: the kernel of call i writes i
    bool timing = false;
    std::vector<hipEvent_t> events;  // start/stop pairs not yet read back
    double timed_ms = 0.0;
    uint64_t timed_launches = 0;
    double build_ms[kReadsBuildStages] = {};  // the stages of the last build from reads
    uint64_t build_pieces = 0;
    double merge_ms[kMergeStages] = {};       // the stages of the last merge
    uint64_t merge_iterations = 0;
    uint64_t spectrum_frontier = 0;           // most nodes per frontier buffer of the k-mer walks (0 = automatic): msbwt_rle_set_spectrum_frontier
    uint64_t spectrum_info[MSBWT_SPECTRUM_INFO_WORDS] = {};  // what the last of them did
    uint64_t spectrum_scratch = 0;            // and the bytes of scratch it allocated (and freed again): msbwt_rle_spectrum_scratch_bytes
    uint64_t unitig_info[MSBWT_UNITIG_INFO_WORDS] = {};  // what the last unitig call found: msbwt_rle_unitig_info
    uint64_t canonical_unitig_info[MSBWT_CANONICAL_UNITIG_INFO_WORDS] = {};  // and the last canonical one: msbwt_rle_canonical_unitig_info
    uint64_t trace_piece = 0;                 // most walks a trace call advances at once (0 = automatic): msbwt_rle_set_trace_piece
    uint64_t trace_info[MSBWT_TRACE_INFO_WORDS] = {};  // what the last trace call did: msbwt_rle_trace_info
    uint64_t canonical_trace_info[MSBWT_CANONICAL_TRACE_INFO_WORDS] = {};  // and the last canonical one: msbwt_rle_canonical_trace_info
    uint64_t walk_piece = 0;                  // most left walks a launch takes (0 = automatic): msbwt_rle_set_walk_piece
    uint64_t walk_info[MSBWT_WALK_INFO_WORDS] = {};  // what the last left-walk call did: msbwt_rle_walk_info
    uint64_t overlap_piece = 0;               // most overlap queries a launch takes (0 = automatic): msbwt_rle_set_overlap_piece
    uint64_t overlap_info[MSBWT_OVERLAP_INFO_WORDS] = {};  // what the last read-overlap call did: msbwt_rle_overlap_info
    uint64_t bridge_slots = 0;                // the frontier slots of a bridge call's piece (0 = automatic): msbwt_rle_set_bridge_slots
    uint64_t bridge_info[MSBWT_BRIDGE_INFO_WORDS] = {};  // what the last bridge call did: msbwt_rle_bridge_info
    std::mutex mu;
    std::string err;
};

namespace msbwt_capi __attribute__((visibility("hidden"))) {

constexpr uint64_t kStreamLinesFrom = uint64_t(4) << 30;  // random-access arrays from here on are read with the non-temporal hint (view_of)

constexpr size_t kStatusBytes = 1024;  // flag words, debug record (bytes 64..128), search counters (bytes 128..256)
constexpr size_t kCountersOffset = 128;
constexpr size_t kSourceBadOffset = 512;  // one u32 of the source index build: a byte >= n_sources was seen
constexpr size_t kPackScratchOffset = 256;  // two u64 of the table packer (escape-line count, side-array cursor)
constexpr size_t kMaxTimedEvents = 256;  // start/stop pairs kept before timed_launch folds them into the running sum
constexpr int kHostFlags = 0, kDeviceFlags = 1;  // words of the status block

// Makes the handle's device current for the scope, restoring the caller's afterwards (the
// caller may be a torch process with its own current device).
class DeviceScope {
  public:
    explicit DeviceScope(int device) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != device) {
            err_ = hipSetDevice(device);
            switched_ = err_ == hipSuccess;
        }
        ok_ = err_ == hipSuccess;
    }
    ~DeviceScope() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    bool ok() const { return ok_; }
    std::string why() const { return std::string("no usable HIP device: ") + hipGetErrorString(err_); }

  private:
    hipError_t err_ = hipSuccess;
    int prev_ = 0;
    bool ok_ = false, switched_ = false;
};

int fail(msbwt_rle *h, int code, const std::string &msg);
int hip_fail(msbwt_rle *h, hipError_t e, const char *what);

#define HIP_TRY(h, expr)                                      \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail(h, e_, #expr);  \
    } while (0)

int ensure_runtime(msbwt_rle *h);
int ensure_stage(msbwt_rle *h, size_t bytes);
int read_flags(msbwt_rle *h, hipStream_t stream, int which, uint32_t *flags);
int flags_to_code(msbwt_rle *h, uint32_t flags);
int status_of(msbwt_rle *h, hipStream_t stream, int which);
int drain_timing_events(msbwt_rle *h, bool wait = true);
int launch_count(msbwt_rle *h, const uint8_t *d_kmers, size_t k, size_t n, uint64_t *d_out, hipStream_t stream, int which);
int launch_count_2bit(msbwt_rle *h, const uint64_t *d_packed, size_t k, size_t n, uint64_t *d_out, hipStream_t stream, int which);  // query.cpp: 2-bit words, 1 <= k <= 64
// sources.cpp: the source vector of n_rows rows (from the host through the pinned pipeline, or already in HBM) attached to the loaded index;
// the caller holds h->mu and has made the handle's device current.  Whatever was attached before is gone either way.
int attach_sources(msbwt_rle *h, const uint8_t *host_rows, const uint8_t *device_rows, uint64_t n_rows, size_t n_sources);

inline IndexView view_of(msbwt_rle *h) {
    IndexView v;
    v.blocks = h->d_blocks;
    v.block_format = h->block_format;
    v.overflow = h->d_overflow;
    v.nblocks = h->nblocks;
    v.total = h->totals.total;
    v.table = h->table.view();
    v.counters = (h->counting && h->d_flags) ? reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(h->d_flags) + kCountersOffset) : nullptr;
    v.pair_blocks = h->pair.blocks;
    v.pair_super = static_cast<const uint64_t *>(h->pair.super);
    v.pair_stride96 = h->pair.blocks && h->pair.stride == 96;
    v.search_kernel = h->search_kernel;
    {   // lines used once should not evict what is reused -- once the arrays the search reads at random (pair blocks, else the blocks
        // themselves) are far beyond what L2 (8 x 4 MB) and the Infinity Cache (256 MB) hold: 4 GiB and up
        const uint64_t hot = h->pair.blocks ? h->pair.bytes : h->nblocks * kBlockBytes;
        v.stream_lines = h->wanted_streaming > 0 || (h->wanted_streaming < 0 && hot >= kStreamLinesFrom);
    }
    if (h->sparse.lines && (h->pair.blocks || h->block_format == kBlocksRuns)) {  // (run blocks: built from pair blocks that are gone again)
        v.sparse = h->sparse.view();
        v.sparse2 = h->sparse2.view();
    }
    v.debug = h->d_flags ? reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(h->d_flags) + 64) : nullptr;
    return v;  // tile_counter: with_tickets()
}

// The two-tier form goes on through the direct table (sparse_policy.hpp, sparse_tier_fits_direct): a direct table deeper than a two-tier
// level would wrap the kernel's count of the symbols between the two, and an escape line without its side entry cannot be followed from
// the filter's path.  The loader builds neither; whatever path might, every query launch checks the handle here first and is refused
// (hipErrorInvalidValue) instead of being made.
inline bool tier_launch_ok(const msbwt_rle *h) {
    const DirectTable &t = h->table;
    if (!t.entries) return true;
    const bool unfollowable = t.packed && t.escape_lines > 0 && !t.side;
    auto level_ok = [&](const SparseLevel &s) { return !(s.lines && s.tier) || (sparse_tier_fits_direct(s.depth, t.depth) && !unfollowable); };
    return level_ok(h->sparse) && level_ok(h->sparse2);
}

// Runs `launch(view)` with a ticket-counter block that no launch still in flight uses, and marks the block busy
// until everything enqueued on `stream` so far -- the launch included -- has completed.  The caller holds h->mu.
template <class Launch>
hipError_t with_slot(msbwt_rle *h, hipStream_t stream, Launch &&launch) {
    if (!tier_launch_ok(h)) return hipErrorInvalidValue;
    // Launches queued back to back on ONE stream are ordered by the stream itself (the memset of the counters waits for the
    // previous kernel), so they share a block without asking its event: a caller that enqueues N asynchronous launches
    // gets one block, not N allocations inside its launch path.
    // (NOT for hipStreamPerThread: that one handle value stands for a different queue in every host thread, so two threads' launches
    // "on the same stream" may run side by side -- they go by the completion event like launches on different streams)
    msbwt_rle::TicketSlot *slot = nullptr;
    for (auto &s : h->tickets)
        if (stream != hipStreamPerThread && s.used && s.last_stream == stream) {
            slot = &s;
            break;
        }
    for (auto &s : h->tickets)
        if (!slot && (!s.used || hipEventQuery(s.done) == hipSuccess)) slot = &s;
    (void)hipGetLastError();  // hipErrorNotReady from a busy slot is not an error
    if (!slot) {
        msbwt_rle::TicketSlot fresh;
        hipError_t e = hipMalloc(&fresh.counters, kTicketBytes);
        if (std::getenv("MSBWT_VERBOSE")) std::fprintf(stderr, "[msbwt] launch slot: ticket counters %p\n", fresh.counters);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&fresh.done, hipEventDisableTiming);
        if (e != hipSuccess) {
            if (fresh.counters) (void)hipFree(fresh.counters);
            return e;
        }
        h->tickets.push_back(fresh);
        slot = &h->tickets.back();
    }
    IndexView v = view_of(h);
    v.tile_counter = slot->counters;
    hipError_t e = launch(v, *slot);
    // recorded even after a failed launch: the memset of the counters may already be queued
    const hipError_t r = hipEventRecord(slot->done, stream);
    slot->used = true;
    slot->last_stream = stream;
    return e != hipSuccess ? e : r;
}

template <class Launch>
hipError_t with_tickets(msbwt_rle *h, hipStream_t stream, Launch &&launch) {
    return with_slot(h, stream, [&](const IndexView &v, msbwt_rle::TicketSlot &) { return launch(v); });
}

// Runs `launch` (which enqueues the count kernel on `stream`); when kernel timing is on, brackets
// it with HIP events on that same stream (read back by msbwt_rle_kernel_time_ms).
template <class Launch>
int timed_launch(msbwt_rle *h, hipStream_t stream, Launch &&launch) {
    if (!h->timing) {
        HIP_TRY(h, launch());
        return MSBWT_OK;
    }
    hipEvent_t start = nullptr, stop = nullptr;
    hipError_t e = hipEventCreate(&start);
    if (e == hipSuccess) e = hipEventCreate(&stop);
    if (e == hipSuccess) e = hipEventRecord(start, stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipEventRecord(stop, stream);
    if (e != hipSuccess) {  // nothing is left behind on the error path
        if (start) (void)hipEventDestroy(start);
        if (stop) (void)hipEventDestroy(stop);
        return hip_fail(h, e, "count kernel launch");
    }
    h->events.push_back(start);
    h->events.push_back(stop);
    // a caller that never reads the timer must not grow this forever: completed pairs are folded away without blocking; only a
    // caller with more than 16 x kMaxTimedEvents launches IN FLIGHT is made to wait
    if (h->events.size() >= 2 * kMaxTimedEvents) return drain_timing_events(h, h->events.size() >= 32 * kMaxTimedEvents);
    return MSBWT_OK;
}

// timed_launch of `launch(view)` with ticket counters (with_tickets)
template <class Launch>
int timed_with_tickets(msbwt_rle *h, hipStream_t stream, Launch &&launch) {
    return timed_launch(h, stream, [&] { return with_tickets(h, stream, launch); });
}

// An entry point's prologue: the handle locked for the call, its index checked (loaded), its device made current (bind; open: both).
class Call {
  public:
    msbwt_rle *const h;
    explicit Call(const msbwt_rle *ch) : h(const_cast<msbwt_rle *>(ch)) {
        if (h) lock_ = std::unique_lock<std::mutex>(h->mu);
    }
    int loaded() const { return h->loaded ? MSBWT_OK : fail(h, MSBWT_ERR_NOT_LOADED, "no BWT loaded"); }
    int bind() {
        scope_.emplace(h->device);
        return scope_->ok() ? MSBWT_OK : fail(h, MSBWT_ERR_HIP, scope_->why());
    }
    // null handle, no index, then the caller's own arguments (`bad_args`: refused with `why`), then bind()
    int open(bool bad_args = false, const char *why = nullptr) {
        if (!h) return MSBWT_ERR_INVALID_ARG;
        if (int rc = loaded()) return rc;
        if (bad_args) return fail(h, MSBWT_ERR_INVALID_ARG, why);
        return bind();
    }

  private:
    std::unique_lock<std::mutex> lock_;
    std::optional<DeviceScope> scope_;
};

// The setters of what a loaded index is built from: `assign()` records the wish under the lock and says whether the index must follow
// it; if so and an index is loaded, `rebuild()` runs on the handle's device.
template <class Assign, class Rebuild>
int set_then_rebuild(msbwt_rle *h, Assign &&assign, Rebuild &&rebuild) {
    Call c(h);
    if (!assign() || !h->loaded) return MSBWT_OK;
    if (int rc = c.bind()) return rc;
    return rebuild();
}

// a setting that takes effect at the next launch or load: recorded under the lock
template <class T, class V>
int set_locked(msbwt_rle *h, T &setting, V value) {
    std::lock_guard<std::mutex> lock(h->mu);
    setting = value;
    return MSBWT_OK;
}

}  // namespace msbwt_capi
