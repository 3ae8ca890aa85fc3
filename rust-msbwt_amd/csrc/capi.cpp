// extern "C" boundary (include/msbwt_hip.h): the handle's life, the two plain loads, every setter, getter and info call, the host-only
// utilities, and the out-of-line helpers that handle.hpp declares.  Loader: index_build.cpp; queries: query.cpp; source colouring: sources.cpp; builders and merges:
// produce.cpp; replicas and gathers: multi_device.cpp.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "handle.hpp"
#include "index_build.hpp"
#include "npy_io.hpp"
#include "pair_index.hpp"
#include "plane_index.hpp"
#include "run_index.hpp"
#include "sparse_table.hpp"

namespace {

constexpr int kMaxTableDepth = 16;  // 4^16 x 16 B = 64 GiB
static_assert(MSBWT_SEARCH_COUNTERS == kSearchCounters, "the header's counter block is the kernels'");
static_assert(MSBWT_BUILD_STAGES == kReadsBuildStages, "the header's stage count is the builder's");
static_assert(MSBWT_MERGE_STAGES == kMergeStages, "the header's stage count is the merge's");
static_assert(MSBWT_MERGE_MAX_INPUTS == kMergeMaxInputs, "the header's input count is the merge's");
static_assert(10 + kSparseMaxDepth + 1 <= 42 && 45 + kSparseMaxDepth + 1 <= 80 && 80 + kSparseMaxDepth + 1 <= 112 && 119 <= MSBWT_SPARSE_INFO_WORDS,
              "msbwt_rle_sparse_table_info: [10 + d] distinct, [42] filtered, [45 + d] wide, [80 + d] once, [112] second tier, [113 .. 119) the walks");

const char *kVersion = "rust-msbwt_amd 0.1.0 (gfx950 plane-block index)";

// random 128-byte lines per second the memory system serves from this allocation right now (0: could not be measured)
double line_rate_of(const void *p, size_t bytes, hipStream_t stream) {
    hipEvent_t a = nullptr, b = nullptr;
    uint64_t lines = 0;
    float ms = 0.f;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = launch_probe_lines(p, bytes, 4, nullptr, nullptr, stream);  // warm-up: page tables, clocks
    if (e == hipSuccess) e = hipEventRecord(a, stream);
    if (e == hipSuccess) e = launch_probe_lines(p, bytes, 48, &lines, nullptr, stream);  // 2.5 x 10^7 lines: about 0.6 ms
    if (e == hipSuccess) e = hipEventRecord(b, stream);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (e != hipSuccess || ms <= 0.f) {
        (void)hipGetLastError();
        return 0.0;
    }
    return double(lines) / (double(ms) * 1e-3);
}

// A sparse-table setting changes a loaded plane-block index only when it changes what it would be built as (run blocks: at the next load).
int set_sparse_wish(msbwt_rle *h, int &wish, int mode) {
    return set_then_rebuild(h, [&] {
        const bool changes = mode != wish;
        wish = mode;
        return changes && h->wanted_sparse != 0 && h->block_format == kBlocksPlanes;
    }, [&] { return rebuild_table(h); });
}

int npy_code(NpyStatus s) {
    switch (s) {
        case NpyStatus::kOk: return MSBWT_OK;
        case NpyStatus::kIo: return MSBWT_ERR_IO;
        case NpyStatus::kUnexpectedEof: return MSBWT_ERR_UNEXPECTED_EOF;
        default: return MSBWT_ERR_BAD_HEADER;
    }
}

}  // namespace

namespace msbwt_capi {

int fail(msbwt_rle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}

int hip_fail(msbwt_rle *h, hipError_t e, const char *what) {
    return fail(h, MSBWT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int ensure_runtime(msbwt_rle *h) {
    if (!h->stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    if (!h->d_flags) {
        HIP_TRY(h, hipMalloc(reinterpret_cast<void **>(&h->d_flags), kStatusBytes));
        if (std::getenv("MSBWT_VERBOSE")) std::fprintf(stderr, "[msbwt] status block %p\n", static_cast<void *>(h->d_flags));
        HIP_TRY(h, hipMemset(h->d_flags, 0, kStatusBytes));
    }
    return MSBWT_OK;
}

int ensure_stage(msbwt_rle *h, size_t bytes) {
    if (bytes <= h->stage_bytes) return MSBWT_OK;
    if (h->d_stage) (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->stage_bytes = 0;
    HIP_TRY(h, hipMalloc(&h->d_stage, bytes));
    h->stage_bytes = bytes;
    return MSBWT_OK;
}

// Reads and clears one flag word of the status block on `stream` (synchronises it).
int read_flags(msbwt_rle *h, hipStream_t stream, int which, uint32_t *flags) {
    HIP_TRY(h, hipMemcpyAsync(flags, h->d_flags + which, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipMemsetAsync(h->d_flags + which, 0, sizeof(uint32_t), stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return MSBWT_OK;
}

int flags_to_code(msbwt_rle *h, uint32_t flags) {
    if (flags & kFlagInternal) {
        uint64_t rec[8] = {0};
        (void)hipMemcpy(rec, reinterpret_cast<char *>(h->d_flags) + 64, sizeof rec, hipMemcpyDeviceToHost);
        (void)hipMemset(reinterpret_cast<char *>(h->d_flags) + 64, 0, sizeof rec);
        char buf[256];
        std::snprintf(buf, sizeof buf, "device consistency check failed: range [%llu, %llu) outside the index (rem|slot %#llx, symbols %#llx, wave|lane %#llx)",
                      (unsigned long long)rec[1], (unsigned long long)rec[2], (unsigned long long)rec[3], (unsigned long long)rec[4],
                      (unsigned long long)rec[5]);
        return fail(h, MSBWT_ERR_INTERNAL, buf);
    }
    if (flags & kFlagInvalidSymbol) return fail(h, MSBWT_ERR_INVALID_SYMBOL, "a query holds a symbol code >= 6");
    if (flags & kFlagInvalidRange) return fail(h, MSBWT_ERR_INVALID_RANGE, "a range has l > h or h > total size");
    if (flags & kFlagNarrowOverflow) return fail(h, MSBWT_ERR_OVERFLOW, "a count does not fit the wire width of the all-gather: repeat it with 64 bits");
    return MSBWT_OK;
}

// read_flags, then what the word says
int status_of(msbwt_rle *h, hipStream_t stream, int which) {
    uint32_t flags = 0;
    const int rc = read_flags(h, stream, which, &flags);
    return rc ? rc : flags_to_code(h, flags);
}

// Folds the recorded start/stop pairs into the running sum.  wait = true (msbwt_rle_kernel_time_ms): waits for the kernels
// they bracket; wait = false (inside an asynchronous launch): only the pairs whose kernel has completed -- in stream order, so
// stopping at the first pending one loses nothing -- and never blocks the caller.
int drain_timing_events(msbwt_rle *h, bool wait) {
    int rc = MSBWT_OK;
    size_t kept = 0;
    for (size_t i = 0; i + 1 < h->events.size(); i += 2) {
        float ms = 0.f;
        if (!wait && hipEventQuery(h->events[i + 1]) != hipSuccess) {
            (void)hipGetLastError();
            h->events[kept++] = h->events[i];
            h->events[kept++] = h->events[i + 1];
            continue;
        }
        hipError_t e = hipEventSynchronize(h->events[i + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->events[i], h->events[i + 1]);
        if (e == hipSuccess) {
            h->timed_ms += ms;
            h->timed_launches += 1;
        } else if (!rc) {
            rc = hip_fail(h, e, "kernel timing events");
        }
        (void)hipEventDestroy(h->events[i]);
        (void)hipEventDestroy(h->events[i + 1]);
    }
    h->events.resize(kept);
    return rc;
}

}  // namespace msbwt_capi

extern "C" {

const char *msbwt_version(void) { return kVersion; }

msbwt_rle *msbwt_rle_new_on_device(uint8_t bin_power, int device) {
    msbwt_rle *h = new (std::nothrow) msbwt_rle();
    if (!h) return nullptr;
    h->bin_power = bin_power;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    h->device = device;
    if (const char *env = std::getenv("MSBWT_TABLE_DEPTH")) h->wanted_table_depth = std::max(-1, std::min(std::atoi(env), kMaxTableDepth));
    if (const char *env = std::getenv("MSBWT_TABLE_PACKED")) h->wanted_table_packed = std::atoi(env) ? 1 : 0;
    if (const char *env = std::getenv("MSBWT_TABLE_SIDE")) h->wanted_table_side = std::atoi(env) ? 1 : 0;
    if (const char *env = std::getenv("MSBWT_STREAM_LINES")) h->wanted_streaming = std::strcmp(env, "auto") == 0 ? -1 : (std::atoi(env) ? 1 : 0);
    if (const char *env = std::getenv("MSBWT_QUERY_K")) h->query_length = std::max(0, std::atoi(env));
    if (const char *env = std::getenv("MSBWT_SPARSE_TABLE")) {
        const int d = std::strcmp(env, "auto") == 0 ? -1 : std::atoi(env);
        h->wanted_sparse = (d == 0 || d == -1 || (d >= kSparseMinDepth && d <= kSparseMaxDepth)) ? d : -1;
    }
    if (const char *env = std::getenv("MSBWT_SPARSE_SECOND")) h->wanted_second = std::strcmp(env, "auto") == 0 ? -1 : (std::atoi(env) ? -1 : 0);
    if (const char *env = std::getenv("MSBWT_SPARSE_TIERS")) h->wanted_tiers = std::strcmp(env, "auto") == 0 ? -1 : (std::atoi(env) ? 1 : 0);
    if (const char *env = std::getenv("MSBWT_PAIR_INDEX")) h->wanted_pair = std::atoi(env) ? 1 : 0;
    if (const char *env = std::getenv("MSBWT_PAIR_STRIDE")) h->wanted_pair_stride = std::atoi(env);
    if (const char *env = std::getenv("MSBWT_FILTER")) h->wanted_filter = std::atoi(env) ? -1 : 0;
    if (const char *env = std::getenv("MSBWT_BLOCKS")) h->wanted_block_format = std::strcmp(env, "runs") == 0 ? kBlocksRuns : kBlocksPlanes;
    if (const char *env = std::getenv("MSBWT_MEMORY_BUDGET")) h->memory_budget = std::strtoull(env, nullptr, 10);
    if (const char *env = std::getenv("MSBWT_ORDER")) h->wanted_order = std::strcmp(env, "auto") == 0 ? -1 : (std::atoi(env) ? 1 : 0);
    if (const char *env = std::getenv("MSBWT_BUILD_PIECE")) h->build_piece = std::strtoull(env, nullptr, 10);
    if (const char *env = std::getenv("MSBWT_ORDER_BITS")) h->order_bits = std::max(1, std::min(std::atoi(env), 36));
    if (const char *env = std::getenv("MSBWT_SEARCH"))
        h->search_kernel = std::strcmp(env, "groups") == 0 ? kSearchGroups : std::strcmp(env, "lanes") == 0 ? kSearchLanes : kSearchAuto;
    return h;
}

msbwt_rle *msbwt_rle_new(uint8_t bin_power) { return msbwt_rle_new_on_device(bin_power, -1); }

void msbwt_rle_free(msbwt_rle *h) {
    if (!h) return;
    {
        DeviceScope scope(h->device);
        release_index(h);
        for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
        for (auto &t : h->tickets) {
            if (t.done) (void)hipEventDestroy(t.done);
            if (t.counters) (void)hipFree(t.counters);
            if (t.order_scratch) (void)hipFree(t.order_scratch);
            if (t.range_scratch) (void)hipFree(t.range_scratch);
        }
        h->pipe.release();
        if (h->mail) (void)hipHostFree(h->mail);
        if (h->d_gather) (void)hipFree(h->d_gather);
        for (hipEvent_t e : h->piece_events) (void)hipEventDestroy(e);
        if (h->gather_stream) (void)hipStreamDestroy(h->gather_stream);
        if (h->d_stage) (void)hipFree(h->d_stage);
        if (h->d_flags) (void)hipFree(h->d_flags);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

int msbwt_rle_load_vector(msbwt_rle *h, const uint8_t *rle_bytes, size_t len) {
    if (!h || (!rle_bytes && len)) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return install(h, rle_bytes, len);
}

int msbwt_rle_load_numpy_file(msbwt_rle *h, const char *utf8_path) {
    if (!h || !utf8_path) return MSBWT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    MappedPayload payload;  // mapped, not read: the upload reads it straight from the page cache
    std::string msg;
    switch (map_npy_payload(utf8_path, &payload, &msg)) {
        case NpyStatus::kOk: break;
        case NpyStatus::kIo: return fail(h, MSBWT_ERR_IO, msg);
        case NpyStatus::kUnexpectedEof: return fail(h, MSBWT_ERR_UNEXPECTED_EOF, msg);
        case NpyStatus::kBadHeader: return fail(h, MSBWT_ERR_BAD_HEADER, msg);
    }
    return install(h, payload.data(), payload.size());
}

uint64_t msbwt_rle_get_symbol_count(const msbwt_rle *h, uint8_t symbol) {
    return (h && symbol < kAlphabet) ? h->totals.symbol_counts[symbol] : 0;
}

uint64_t msbwt_rle_get_total_size(const msbwt_rle *h) { return h ? h->totals.total : 0; }

int msbwt_rle_set_table_depth(msbwt_rle *h, int depth) {
    if (!h || depth > kMaxTableDepth) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->wanted_table_depth = depth; return true; }, [&] { return rebuild_table(h); });
}

int msbwt_rle_get_table_depth(const msbwt_rle *h) { return h ? h->table.depth : 0; }

int msbwt_rle_set_pair_index(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->wanted_pair = mode; return true; }, [&] { return rebuild_pair_and_table(h); });
}

int msbwt_rle_get_pair_index(const msbwt_rle *h) { return (h && h->pair.blocks) ? 1 : 0; }

int msbwt_rle_set_pair_stride(msbwt_rle *h, int stride) {
    if (!h || (stride != 0 && stride != 96 && stride != 128)) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->wanted_pair_stride = stride; return true; }, [&] { return rebuild_pair_and_table(h); });
}

int msbwt_rle_get_pair_stride(const msbwt_rle *h) { return (h && h->pair.blocks) ? h->pair.stride : 0; }

int msbwt_rle_set_presence_filter(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    // (the filter is made from the flat table, which a packed table no longer holds)
    return set_then_rebuild(h, [&] { h->wanted_filter = mode == 0 ? 0 : -1; return true; }, [&] { return rebuild_table(h); });
}

int msbwt_rle_set_table_packed(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->wanted_table_packed = mode; return true; }, [&] { return rebuild_table(h); });
}

int msbwt_rle_get_table_packed(const msbwt_rle *h) { return (h && h->table.entries && h->table.packed) ? 1 : 0; }

int msbwt_rle_set_memory_budget(msbwt_rle *h, uint64_t bytes) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->memory_budget = bytes; return true; }, [&] {
        if (int rc = replan(h, bytes)) return rc;  // the optional structures are rebuilt under the new budget
        // a budget that cannot be met is said, not silently exceeded (the call still succeeds: the index works)
        h->err.clear();
        if (bytes != 0 && h->block_format != kBlocksPlanes) h->err = "memory budget: the run-block format has no optional structures to plan; the budget is not applied";
        else if (bytes != 0 && bytes < h->nblocks * kBlockBytes) h->err = "memory budget: below the plane blocks themselves, which are built all the same";
        return int(MSBWT_OK);
    });
}

uint64_t msbwt_rle_get_memory_budget(const msbwt_rle *h) { return h ? h->memory_budget : 0; }

int msbwt_auto_index_plan(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t hbm_total_bytes, double typical_width, uint64_t budget_bytes,
                          int *pair_index, int *pair_stride, int *flat_depth, int *packed_depth, uint64_t *index_bytes) {
    if (!pair_index || !pair_stride || !flat_depth || !packed_depth) return MSBWT_ERR_INVALID_ARG;
    const uint64_t nblocks = plane_block_count(total_symbols);
    const PairIndexSizes wide = pair_index_sizes(nblocks, 96), narrow = pair_index_sizes(nblocks, 128);
    const IndexPlan p = plan_index(total_symbols, free_hbm_bytes, hbm_total_bytes, typical_width, budget_bytes, narrow.pair_block_bytes + narrow.super_bytes,
                                   wide.pair_block_bytes + wide.super_bytes);
    *pair_index = p.pair ? 1 : 0;
    *pair_stride = p.pair ? p.stride : 0;
    *flat_depth = p.flat;
    *packed_depth = p.packed;
    if (index_bytes) *index_bytes = p.bytes;
    return MSBWT_OK;
}

int msbwt_rle_set_table_side(msbwt_rle *h, int mode) {
    if (!h || mode < 0 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->wanted_table_side = mode; return true; }, [&] { return rebuild_table(h); });
}

int msbwt_rle_table_info(const msbwt_rle *h, uint64_t *lines, uint64_t *escape_lines, uint64_t *side_bytes) {
    if (!h) return MSBWT_ERR_INVALID_ARG;
    const DirectTable &t = h->table;
    const bool packed = t.entries && t.packed;
    if (lines) *lines = packed ? t.lines : 0;
    if (escape_lines) *escape_lines = packed ? t.escape_lines : 0;
    if (side_bytes) *side_bytes = packed ? t.side_bytes : 0;
    return MSBWT_OK;
}

// ---- sparse suffix table (sparse_table.hpp) ----------------------------------------------------------------------------------
int msbwt_rle_set_sparse_table(msbwt_rle *h, int depth) {
    if (!h || !(depth == -1 || depth == 0 || (depth >= kSparseMinDepth && depth <= kSparseMaxDepth))) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] { h->wanted_sparse = depth; return true; }, [&] {
        if (h->block_format != kBlocksPlanes) {  // run blocks: the table is built at load time only (from plane blocks that are gone); 0 drops it now
            if (depth == 0) release_sparse(h);
            return int(MSBWT_OK);
        }
        return rebuild_table(h);
    });
}

int msbwt_rle_get_sparse_table(const msbwt_rle *h) { return (h && h->sparse.lines) ? h->sparse.depth : 0; }

int msbwt_rle_set_sparse_tiers(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    return set_sparse_wish(h, h->wanted_tiers, mode);
}

int msbwt_rle_get_sparse_tiers(const msbwt_rle *h) { return (h && h->sparse.lines && h->sparse.tier) ? 1 : 0; }

int msbwt_rle_set_sparse_second(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 0) return MSBWT_ERR_INVALID_ARG;
    return set_sparse_wish(h, h->wanted_second, mode);
}

int msbwt_rle_set_query_length(msbwt_rle *h, int k) {
    if (!h || k < 0) return MSBWT_ERR_INVALID_ARG;
    return set_then_rebuild(h, [&] {
        const bool changes = sparse_auto_max_depth(k) != sparse_auto_max_depth(h->query_length);
        h->query_length = k;
        return changes && h->wanted_sparse < 0 && h->block_format == kBlocksPlanes;  // (an explicit depth, or none at all, does not follow the hint)
    }, [&] { return rebuild_table(h); });
}

int msbwt_rle_get_query_length(const msbwt_rle *h) { return h ? h->query_length : 0; }

int msbwt_auto_sparse_max_depth(int query_length) { return sparse_auto_max_depth(query_length); }

int msbwt_rle_sparse_table_info(const msbwt_rle *ch, uint64_t *out) {
    if (!ch || !out) return MSBWT_ERR_INVALID_ARG;
    Call c(ch);
    std::memset(out, 0, MSBWT_SPARSE_INFO_WORDS * sizeof(uint64_t));
    const SparseBuildReport &r = c.h->sparse_report;
    const SparseLevel &s = c.h->sparse, &s2 = c.h->sparse2;
    if (s.lines) {
        out[0] = uint64_t(s.depth);
        out[1] = r.entries;
        out[2] = s.nbuckets;
        out[3] = s.bytes;
        out[4] = r.nescapes;
        out[5] = s.side_bytes;
        out[6] = r.displaced;
        out[8] = s.tier ? 1 : 0;
        out[9] = s.probe;
        out[42] = r.filtered;
        out[43] = uint64_t(s2.depth);
        out[44] = s2.bytes + s2.side_bytes;
        out[112] = s2.lines && s2.tier ? 1 : 0;
    }
    out[7] = uint64_t(r.parent_depth);
    for (int d = 0; d <= kSparseMaxDepth; ++d) {
        out[10 + d] = r.distinct[d];
        out[45 + d] = r.escapes[d];
        out[80 + d] = r.singles[d];
    }
    for (int j = 0; j < 3; ++j) {
        out[113 + j] = r.sizing_walk[j];
        out[116 + j] = r.fill_walk[j];
    }
    return MSBWT_OK;
}

int msbwt_sparse_hash(uint64_t key, int depth, uint64_t nbuckets, uint32_t *bucket, uint32_t *tag) {
    if (depth < kSparseMinDepth || depth > kSparseMaxDepth || nbuckets == 0 || nbuckets > 0xFFFFFFFFull || !bucket || !tag) return MSBWT_ERR_INVALID_ARG;
    const uint64_t x = sparse_mix(key, uint32_t(2 * depth));
    *bucket = sparse_bucket(x, uint32_t(2 * depth), uint32_t(nbuckets));
    *tag = sparse_tag(x, sparse_layout(uint32_t(depth)));
    return MSBWT_OK;
}

int msbwt_sparse_hash64(uint64_t key, int depth, uint64_t nbuckets, uint32_t *bucket, uint64_t *tag) {
    if (depth < kSparseMinDepth || depth > kSparseMaxDepth || nbuckets == 0 || nbuckets > 0xFFFFFFFFull || !bucket || !tag) return MSBWT_ERR_INVALID_ARG;
    const uint64_t x = sparse_mix(key, uint32_t(2 * depth));
    *bucket = sparse_bucket(x, uint32_t(2 * depth), uint32_t(nbuckets));
    *tag = (uint64_t(sparse_tag_hi(x, sparse_layout(uint32_t(depth)))) << 32) | sparse_tag(x, sparse_layout(uint32_t(depth)));
    return MSBWT_OK;
}

int msbwt_auto_sparse_depth(const uint64_t *distinct, const uint64_t *wide, int parent_depth, uint64_t avail_bytes, int query_length, int *depth, uint64_t *table_bytes) {
    if (!distinct || !wide || !depth || parent_depth < 0 || parent_depth > 16 || query_length < 0) return MSBWT_ERR_INVALID_ARG;
    const SparseChoice c = choose_sparse_depth(distinct, wide, parent_depth, sparse_auto_max_depth(query_length), avail_bytes, 0);
    *depth = c.depth;
    if (table_bytes) *table_bytes = c.bytes;
    return MSBWT_OK;
}

int msbwt_auto_sparse_choice(const uint64_t *distinct, const uint64_t *wide, const uint64_t *singles, int parent_depth, uint64_t avail_bytes, int query_length,
                             int tiers, int *depth, int *two_tier, uint64_t *table_bytes) {
    if (!distinct || !wide || !singles || !depth || !two_tier || parent_depth < 0 || parent_depth > 16 || query_length < 0 || tiers < -1 || tiers > 1)
        return MSBWT_ERR_INVALID_ARG;
    const SparseChoice c = choose_sparse_depth(distinct, wide, parent_depth, sparse_auto_max_depth(query_length), avail_bytes, 0, singles, tiers);
    *depth = c.depth;
    *two_tier = c.tier ? 1 : 0;
    if (table_bytes) *table_bytes = c.bytes;
    return MSBWT_OK;
}

int msbwt_sparse_filter_bits(uint64_t tag, uint32_t *word, uint32_t *mask) {
    if (!word || !mask) return MSBWT_ERR_INVALID_ARG;
    const uint32_t f = sparse_filter_hash(uint32_t(tag));
    *word = sparse_filter_word(f);
    *mask = sparse_filter_mask(f);
    return MSBWT_OK;
}

int msbwt_sparse_table_shape(int depth, uint64_t entries, uint64_t *nbuckets, int *probe) {
    if (depth < kSparseMinDepth || depth > kSparseMaxDepth || !nbuckets || !probe) return MSBWT_ERR_INVALID_ARG;
    *nbuckets = sparse_buckets_for(depth, entries);
    *probe = sparse_probe_limit(depth, *nbuckets);
    return MSBWT_OK;
}

size_t msbwt_rle_download_sparse_table(const msbwt_rle *ch, void *out_lines, size_t cap_bytes, void *out_side, size_t cap_side_bytes) {
    msbwt_rle *h = const_cast<msbwt_rle *>(ch);
    if (!h) return SIZE_MAX;
    std::lock_guard<std::mutex> lock(h->mu);
    const SparseLevel &s = h->sparse;
    if (!h->loaded || !s.lines) return SIZE_MAX;
    DeviceScope scope(h->device);
    if (!scope.ok()) return SIZE_MAX;
    if (out_lines && cap_bytes >= s.bytes && hipMemcpy(out_lines, s.lines, s.bytes, hipMemcpyDeviceToHost) != hipSuccess) return SIZE_MAX;
    if (out_side && s.side && cap_side_bytes >= s.side_bytes && hipMemcpy(out_side, s.side, s.side_bytes, hipMemcpyDeviceToHost) != hipSuccess) return SIZE_MAX;
    return size_t(s.bytes);
}

int msbwt_rle_set_line_streaming(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    return set_locked(h, h->wanted_streaming, mode);
}

int msbwt_rle_get_line_streaming(const msbwt_rle *ch) {
    if (!ch || !ch->loaded) return 0;
    Call c(ch);
    return view_of(c.h).stream_lines ? 1 : 0;
}

int msbwt_rle_probe_line_rate(const msbwt_rle *ch, int which, double *lines_per_second) {
    if (!ch || !lines_per_second || which < 0 || which > 3) return MSBWT_ERR_INVALID_ARG;
    Call c(ch);
    if (int rc = c.open()) return rc;
    msbwt_rle *h = c.h;
    const void *p = which == 0 ? h->d_blocks : which == 1 ? h->pair.blocks : which == 2 ? h->sparse.lines : h->table.entries;
    const uint64_t bytes = which == 0 ? h->nblocks * kBlockBytes : which == 1 ? pair_index_sizes(h->nblocks, h->pair.stride).pair_block_bytes
                           : which == 2 ? h->sparse.bytes : uint64_t(h->table.bytes);
    *lines_per_second = 0.0;
    if (!p || bytes < 128) return MSBWT_OK;
    *lines_per_second = line_rate_of(p, bytes, h->stream);
    return MSBWT_OK;
}

int msbwt_rle_set_search_counters(msbwt_rle *h, int enabled) {
    return h ? set_locked(h, h->counting, enabled != 0) : MSBWT_ERR_INVALID_ARG;
}

int msbwt_rle_search_counters(const msbwt_rle *ch, uint64_t *out, void *hip_stream) {
    if (!ch || !out) return MSBWT_ERR_INVALID_ARG;
    Call c(ch);
    msbwt_rle *h = c.h;
    std::memset(out, 0, MSBWT_SEARCH_COUNTERS * sizeof(uint64_t));
    if (!h->d_flags) return MSBWT_OK;
    if (int rc = c.bind()) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    char *d_counters = reinterpret_cast<char *>(h->d_flags) + kCountersOffset;
    HIP_TRY(h, hipMemcpyAsync(out, d_counters, MSBWT_SEARCH_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipMemsetAsync(d_counters, 0, MSBWT_SEARCH_COUNTERS * sizeof(uint64_t), stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return MSBWT_OK;
}

int msbwt_rle_get_presence_filter(const msbwt_rle *h) { return (h && h->table.filter) ? h->table.filter_depth : 0; }

int msbwt_rle_set_block_format(msbwt_rle *h, int format) {
    if (!h || (format != kBlocksPlanes && format != kBlocksRuns)) return MSBWT_ERR_INVALID_ARG;
    return set_locked(h, h->wanted_block_format, format);  // (the next load builds it)
}

int msbwt_rle_get_block_format(const msbwt_rle *h) { return h ? (h->loaded ? h->block_format : h->wanted_block_format) : 0; }

int msbwt_auto_table_depths(uint64_t total_symbols, uint64_t free_hbm_bytes, int pair_index, int *flat_depth, int *packed_depth) {
    if (!flat_depth || !packed_depth) return MSBWT_ERR_INVALID_ARG;
    const TableChoice c = choose_table_depths(total_symbols, plane_block_count(total_symbols) * kBlockBytes, free_hbm_bytes, pair_index != 0, true);
    *flat_depth = c.flat;
    *packed_depth = c.packed;
    return MSBWT_OK;
}

int msbwt_run_build_fits_device(uint64_t total_symbols, uint64_t free_hbm_bytes) { return run_build_fits_device(total_symbols, free_hbm_bytes) ? 1 : 0; }

int msbwt_auto_pair_stride(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t hbm_total_bytes, double typical_width, int *stride) {
    if (!stride) return MSBWT_ERR_INVALID_ARG;
    const uint64_t nblocks = plane_block_count(total_symbols);
    const PairIndexSizes wide = pair_index_sizes(nblocks, 96), narrow = pair_index_sizes(nblocks, 128);
    const uint64_t bytes96 = wide.pair_block_bytes + wide.super_bytes + wide.scratch_bytes, bytes128 = narrow.pair_block_bytes + narrow.super_bytes;
    const uint64_t after128 = free_hbm_bytes > bytes128 ? free_hbm_bytes - bytes128 : 0;
    *stride = choose_pair_stride(bytes96, expected_table_bytes(total_symbols, nblocks * kBlockBytes, after128, true, true), free_hbm_bytes,
                                 hbm_total_bytes, typical_width);
    return MSBWT_OK;
}

double msbwt_rle_get_typical_range_width(const msbwt_rle *h) { return h ? h->typical_width : -1.0; }

int msbwt_rle_set_search_kernel(msbwt_rle *h, int mode) {
    if (!h || mode < kSearchAuto || mode > kSearchLanes) return MSBWT_ERR_INVALID_ARG;
    return set_locked(h, h->search_kernel, mode);
}

int msbwt_rle_get_search_kernel(const msbwt_rle *h) { return h ? h->search_kernel : 0; }

int msbwt_rle_search_kernel_for(const msbwt_rle *h, size_t k) {
    if (!h || !h->loaded) return MSBWT_ERR_INVALID_ARG;
    if (k > 0xFFFFFFFFull) return 0;
    Call c(h);
    return search_kernel_for(view_of(c.h), uint32_t(k));
}

uint64_t msbwt_rle_device_bytes(const msbwt_rle *h) {
    if (!h || !h->loaded) return 0;
    const DirectTable &t = h->table;
    return h->nblocks * kBlockBytes + h->overflow_bytes + (t.entries ? uint64_t(t.bytes) + t.side_bytes : 0) + h->pair.bytes +
           (t.filter ? (uint64_t(1) << (2 * t.filter_depth)) / 8 : 0) + h->sparse.bytes + h->sparse.side_bytes + h->sparse2.bytes + h->sparse2.side_bytes + h->sources.bytes;
}

int msbwt_rle_set_kernel_timing(msbwt_rle *h, int enabled) {
    return h ? set_locked(h, h->timing, enabled != 0) : MSBWT_ERR_INVALID_ARG;
}

int msbwt_rle_kernel_time_ms(const msbwt_rle *ch, double *avg_ms, uint64_t *launches) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.bind()) return rc;
    const int rc = drain_timing_events(h);
    if (rc) return rc;
    if (avg_ms) *avg_ms = h->timed_launches ? h->timed_ms / double(h->timed_launches) : 0.0;
    if (launches) *launches = h->timed_launches;
    h->timed_ms = 0.0;
    h->timed_launches = 0;
    return MSBWT_OK;
}

int msbwt_rle_device_ordinal(const msbwt_rle *h) { return h ? h->device : -1; }

const char *msbwt_rle_last_error(const msbwt_rle *ch) {
    msbwt_rle *h = const_cast<msbwt_rle *>(ch);
    if (!h) return "null handle";
    // query threads may be failing into h->err right now: copy it under the handle lock into a
    // buffer owned by the calling thread (valid until this thread's next call)
    thread_local std::string mine;
    std::lock_guard<std::mutex> lock(h->mu);
    mine = h->err;
    return mine.c_str();
}

size_t msbwt_rle_download_blocks(const msbwt_rle *ch, void *out_blocks, size_t cap_blocks) {
    msbwt_rle *h = const_cast<msbwt_rle *>(ch);
    if (!h || !h->loaded || h->block_format != kBlocksPlanes) return SIZE_MAX;
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceScope scope(h->device);
    if (!scope.ok()) return SIZE_MAX;
    if (out_blocks && cap_blocks >= h->nblocks &&
        hipMemcpy(out_blocks, h->d_blocks, size_t(h->nblocks) * kBlockBytes, hipMemcpyDeviceToHost) != hipSuccess)
        return SIZE_MAX;
    return size_t(h->nblocks);
}

size_t msbwt_build_plane_blocks(const uint8_t *rle_bytes, size_t len, void *out_blocks, size_t cap_blocks,
                                uint64_t *out_total) {
    Totals t;
    if ((!rle_bytes && len) || !compute_totals(rle_bytes, len, &t) || t.total >= kMaxSymbols) return SIZE_MAX;
    if (out_total) *out_total = t.total;
    const uint64_t nblocks = plane_block_count(t.total);
    if (out_blocks && cap_blocks >= nblocks) build_plane_blocks(rle_bytes, len, t, static_cast<uint32_t *>(out_blocks), 0);
    return size_t(nblocks);
}

size_t msbwt_build_run_blocks(const uint8_t *rle_bytes, size_t len, void *out_blocks, size_t cap_blocks, void *out_overflow,
                              size_t cap_overflow, uint64_t *out_total, uint64_t *out_noverflow) {
    Totals t;
    if ((!rle_bytes && len) || !compute_totals(rle_bytes, len, &t) || t.total >= kMaxSymbols) return SIZE_MAX;
    RunIndex ri;
    build_run_blocks(rle_bytes, len, t, &ri, 0);
    if (out_total) *out_total = t.total;
    if (out_noverflow) *out_noverflow = ri.noverflow;
    if (out_blocks && cap_blocks >= ri.nblocks) std::memcpy(out_blocks, ri.blocks.data(), ri.blocks.size() * sizeof(uint32_t));
    if (out_overflow && cap_overflow >= ri.noverflow && ri.noverflow) std::memcpy(out_overflow, ri.overflow.data(), ri.overflow.size() * sizeof(uint32_t));
    return size_t(ri.nblocks);
}

size_t msbwt_convert_to_vec(const uint8_t *ascii, size_t n, uint8_t *out, size_t cap) {
    std::vector<uint8_t> enc;
    if (!encode_text(ascii, n, &enc)) return SIZE_MAX;
    if (out) std::memcpy(out, enc.data(), std::min(cap, enc.size()));
    return enc.size();
}

int msbwt_save_bwt_numpy(const uint8_t *rle_bytes, size_t n, const char *utf8_path) {
    if (!utf8_path || (!rle_bytes && n)) return MSBWT_ERR_INVALID_ARG;
    std::string msg;
    return npy_code(write_npy_payload(utf8_path, rle_bytes, n, &msg));
}

int msbwt_save_bwt_runs_numpy(const uint8_t *syms, const uint64_t *counts, size_t nruns, const char *utf8_path) {
    if (!utf8_path || (nruns && (!syms || !counts))) return MSBWT_ERR_INVALID_ARG;
    std::vector<uint8_t> enc;
    encode_runs(syms, counts, nruns, &enc);
    std::string msg;
    return npy_code(write_npy_payload(utf8_path, enc.data(), enc.size(), &msg));
}

void msbwt_convert_stoi(const uint8_t *ascii, size_t n, uint8_t *out_codes) { ascii_to_codes(ascii, n, out_codes); }
void msbwt_convert_itos(const uint8_t *codes, size_t n, uint8_t *out_ascii) { codes_to_ascii(codes, n, out_ascii); }
void msbwt_reverse_complement_i(const uint8_t *codes, size_t n, uint8_t *out_codes) {
    reverse_complement_codes(codes, n, out_codes);
}

}  // extern "C"
