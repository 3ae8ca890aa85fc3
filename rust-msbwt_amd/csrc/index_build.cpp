// The index loader: plane and run blocks, pair index, direct, packed and sparse tables, and the memory plan -- what sits in HBM and why.
// The other units reach it through index_build.hpp only; it calls the kernels' host launchers and the shared helpers of handle.hpp.
#include "index_build.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "device_build.hpp"
#include "handle.hpp"
#include "pair_index.hpp"
#include "plane_index.hpp"
#include "rle_subruns.hpp"
#include "run_build.hpp"
#include "run_index.hpp"

namespace {

// One owner for a device temporary: freed when its scope ends, unless release() has handed the pointer to a part of the handle first.
// (What is alive when the loader reads the free HBM decides what it builds: a buffer's scope is part of the policy.)
class DeviceBuf {
  public:
    explicit DeviceBuf(void *adopted = nullptr) : p_(adopted) {}
    DeviceBuf(DeviceBuf &&o) noexcept : p_(o.release()) {}  // (move-only: no copies)
    ~DeviceBuf() { reset(); }
    hipError_t alloc(size_t bytes) {
        reset();
        return hipMalloc(&p_, bytes);
    }
    void reset() { if (void *p = release()) (void)hipFree(p); }
    void *get() const { return p_; }
    void *release() { return std::exchange(p_, nullptr); }

  private:
    void *p_ = nullptr;
};

// MSBWT_VERBOSE=1: one stderr line per load stage and per decision of the loader
bool verbose() { return std::getenv("MSBWT_VERBOSE") != nullptr; }

// MSBWT_BUILD=host: the blocks are built on the host and uploaded (kept for cross-checking the device builder)
bool build_on_host_wanted() {
    const char *mode = std::getenv("MSBWT_BUILD");
    return mode && std::strcmp(mode, "host") == 0;
}

// free HBM beyond `keep_free` and the eighth of the device that stays free for the caller's batches (0: none, or it cannot be told)
uint64_t free_beyond_reserve(uint64_t keep_free) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
    const uint64_t spare = keep_free + total_b / 8;
    return uint64_t(free_b) > spare ? uint64_t(free_b) - spare : 0;
}

// what the memory budget leaves once `held` bytes are paid for
uint64_t budget_left(const msbwt_rle *h, uint64_t held) { return h->memory_budget > held ? h->memory_budget - held : 0; }

// the totals of a stream the host builds from, counted on the host: a bad symbol or 2^40 symbols and more are refused
int host_totals(msbwt_rle *h, const uint8_t *rle, size_t n, Totals *t) {
    if (!compute_totals(rle, n, t)) return fail(h, MSBWT_ERR_INVALID_SYMBOL, "RLE stream holds a symbol code >= 6");
    if (t->total >= kMaxSymbols) return fail(h, MSBWT_ERR_TOO_LARGE, "BWT has 2^40 symbols or more");
    return MSBWT_OK;
}

// two u64 in the status block: the table packer's escape-line count and side-array cursor, or the run-block builder's overflow count
unsigned long long *pack_scratch(const msbwt_rle *h) {
    return reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(h->d_flags) + kPackScratchOffset);
}

// overflow blocks the run blocks made from `planes` need (run_build.hip); the count stays in pack_scratch for launch_run_block_write
hipError_t count_overflow_blocks(msbwt_rle *h, const void *planes, uint64_t nplanes, uint64_t total, unsigned long long *nover) {
    hipError_t e = launch_run_block_count(planes, nplanes, total, pack_scratch(h), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(nover, pack_scratch(h), sizeof *nover, hipMemcpyDeviceToHost, h->stream);
    return e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
}

// Presence filter over the finished table: 4^min(12, depth) bits (<= 2 MiB, L2-sized).  Kept
// only if it can reject something (less than 90 % of its bits set) -- on a large genome every
// 12-mer occurs and the filter would be a wasted lookup.
int rebuild_filter(msbwt_rle *h) {
    DirectTable &t = h->table;
    t.release_filter();
    if (!t.entries || h->wanted_filter == 0 || t.depth < 6) return MSBWT_OK;
    const int fd = std::min(12, t.depth);
    const size_t words = (size_t(1) << (2 * fd)) / 32;
    DeviceBuf filter;
    HIP_TRY(h, filter.alloc(words * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(filter.get(), 0, words * sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = launch_build_filter(t.entries, t.depth, fd, static_cast<uint32_t *>(filter.get()), h->stream);
    std::vector<uint32_t> host(words);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), filter.get(), words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_fail(h, e, "build presence filter");
    uint64_t set = 0;
    for (uint32_t w : host) set += uint64_t(__builtin_popcount(w));
    if (double(set) > 0.9 * double(words * 32)) return MSBWT_OK;
    t.filter = static_cast<uint32_t *>(filter.release());
    t.filter_depth = fd;
    return MSBWT_OK;
}

// A flat direct table of `depth` levels from the index in HBM: allocated, built and waited for.  *out is written on success only; what a
// failure means is the caller's policy.
hipError_t build_flat_table(msbwt_rle *h, int depth, DirectTable *out) {
    const size_t bytes = (size_t(1) << (2 * depth)) * 16;
    DeviceBuf tab;
    hipError_t e = tab.alloc(bytes);
    if (e == hipSuccess) e = launch_build_table(view_of(h), depth, tab.get(), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return e;
    out->entries = tab.release();  // (*out is a released table: flat, without side array or filter)
    out->depth = depth;
    out->bytes = bytes;
    return hipSuccess;
}

// Sparse suffix table (sparse_table.hpp) from the flat direct table that is in HBM right now (its parent; none: from the root).
// Optional structure: when nothing fits (or a step fails for want of memory) the handle simply has none -- unless a depth was
// asked for explicitly, which is then an error.  keep_free: bytes that what is built afterwards (the packed direct table) still
// needs; allowance: what a memory budget leaves for this table (kNoBudget: none in force).
// direct_depth: the depth the direct table will have once the sparse table is built (packed: two deeper than the flat one in HBM now; 0 =
// none) -- a two-tier level may not be shallower (sparse_tier_fits_direct).
// deep_direct_depth: the flat depth of the DEEP direct table that is kept beside the sparse table when HBM is plentiful (build_tables; 0 =
// not in question) -- where that one fits no second sparse level is built.
constexpr int kSparseSecondDepth = 17;  // entries of the second, shallower level (what the packed direct table of round 4 reached)

bool deep_direct_fits(const msbwt_rle *h, int flat_depth_wanted) {
    if (flat_depth_wanted <= 0 || flat_depth_wanted + 2 > 18 || h->planned) return false;
    size_t free_b = 0, total_b = 0;
    const uint64_t flat_deep = (uint64_t(1) << (2 * flat_depth_wanted)) * 16, packed = packed_table_bytes(flat_depth_wanted + 2);
    const uint64_t need = flat_deep + packed + packed / 8;  // (the packer's side array of escape lines: an eighth at most in practice)
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && uint64_t(free_b) + h->table.bytes >= need + uint64_t(total_b) / 8;
}

// what the fill passes of both levels share: the parent table the expansion starts from (nullptr: from the root, depth 0) and the work
// scratch of the sizing pass
struct SparseWork { const void *flat; int flat_depth; void *work; size_t work_bytes; };

// One level of the sparse table, filled as `choice` says (rep: the sizing pass's report, IN and OUT as for sparse_fill): side array, bucket lines and slot counters are allocated, sparse_fill runs, *out owns lines and side.
// An entry without a slot within the probe limit (hipErrorInvalidValue) gets a quarter more buckets, `attempts` fills at most, while the
// grown table still fits `limit` bytes.  `counts` is the caller's: it decides how long the slot counters stay allocated.  On failure
// *what names the step.
hipError_t fill_sparse_level(msbwt_rle *h, const SparseWork &w, const SparseChoice &choice, SparseBuildReport *rep, int attempts, uint64_t limit, DeviceBuf *counts,
                             SparseLevel *out, const char **what) {
    const uint64_t nside = rep->escapes[choice.depth];
    uint64_t nbuckets = choice.nbuckets;
    DeviceBuf side, lines;
    auto failed = [&](hipError_t e, const char *step) {
        *what = step;
        return e;
    };
    hipError_t e = nside ? side.alloc(nside * 16) : hipSuccess;
    if (e != hipSuccess) return failed(e, "side array");
    for (int attempt = 1;; ++attempt) {
        const int probe = sparse_probe_limit(choice.depth, nbuckets);
        if (probe < 1) return failed(hipErrorInvalidValue, "bucket count");
        const uint64_t nlines = nbuckets + uint64_t(probe);
        e = lines.alloc(nlines * 128);
        if (e == hipSuccess) e = counts->alloc(nlines * sizeof(uint32_t));
        if (e != hipSuccess) return failed(e, "bucket lines");
        e = sparse_fill(view_of(h), w.flat, w.flat_depth, choice.depth, choice.tier, lines.get(), nbuckets, uint32_t(probe), side.get(), nside, counts->get(), w.work, w.work_bytes, rep, h->stream);
        if (e == hipSuccess) {
            *out = SparseLevel{lines.release(), side.release(), nlines * 128, nside * 16, 0, uint32_t(nbuckets), uint32_t(probe), choice.depth, choice.tier};
            return hipSuccess;
        }
        if (e != hipErrorInvalidValue || attempt == attempts) return failed(e, "fill pass");
        lines.reset();  // some entry found no slot within the probe limit: a quarter more buckets
        counts->reset();
        nbuckets += nbuckets / 4;
        // the larger table must still fit what the first one was chosen within (the budget, the eighth of HBM left to the caller) and the format
        const uint64_t again = nbuckets + kSparseMaxProbe;
        if (again > 0xFFFFFFFFull || again * 128 + again * sizeof(uint32_t) + nside * 16 > limit) return failed(hipErrorOutOfMemory, "fill pass (no room for more buckets)");
    }
}

// ---- a second, shallower level for the queries the first table is too deep for (sparse_for, kernels.hpp) -----------------------------
// With k undeclared the first table is 23 deep and k = 17..22 fall to the direct table, which stays at packed depth 15 beside a sparse
// table: measured at human scale (round 6, present k-mers), k = 17 / 19 / 21 run 2.5 / 1.8 / 1.5 x slower than on the index WITHOUT a
// sparse table (packed depth 17).  Where the deep direct table itself fits (build_tables keeps it then) nothing is needed; otherwise the
// same sizing counts fill a table of the suffixes of 17 symbols -- when it fits what is left, an eighth of the device still
// free.  A declared k gets none (the caller has said what it will ask), an explicit depth neither.
// (run blocks are the memory-lean format: no second level there)
// Optional: an entry without a slot, no memory -- the index simply has no second level.  Sized and filled while the first level's work
// scratch and slot counters are still allocated (build_sparse holds them).
void build_second_sparse_level(msbwt_rle *h, const SparseWork &w, const SparseBuildReport &rep, int tiers, int direct_depth, int deep_direct_depth, uint64_t keep_free,
                               uint64_t allowance) {
    if (h->wanted_sparse > 0 || h->wanted_second == 0 || h->wanted_block_format != kBlocksPlanes || h->query_length != 0 || h->sparse.depth <= kSparseSecondDepth ||
        deep_direct_fits(h, deep_direct_depth))
        return;
    const uint64_t used = h->sparse.bytes + h->sparse.side_bytes;
    const uint64_t avail = std::min<uint64_t>(allowance > used ? allowance - used : 0, free_beyond_reserve(keep_free));
    const SparseChoice second = choose_sparse_depth(rep.distinct, rep.escapes, w.flat_depth, std::min(kSparseSecondDepth, h->sparse.depth - 1), avail, 0, rep.singles, tiers, direct_depth);
    if (!second.depth) return;
    DeviceBuf counts;  // (its own buffers: the first table's are the handle's by now)
    SparseBuildReport rep2 = rep;
    const char *what = "";
    const hipError_t e = fill_sparse_level(h, w, second, &rep2, 1, kNoBudget, &counts, &h->sparse2, &what);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (verbose()) std::fprintf(stderr, "[msbwt] sparse table, second level: %s -- none built\n", hipGetErrorString(e));
        return;
    }
    SparseLevel &s = h->sparse2;
    s.entries = rep2.entries;
    if (verbose())
        std::fprintf(stderr, "[msbwt] sparse table, second level: depth %d%s, %llu entries in %u buckets, %.2f GB (serves %d <= k < %d)\n", s.depth, s.tier ? " two-tier" : "",
                     (unsigned long long)s.entries, s.nbuckets, double(s.bytes + s.side_bytes) / 1e9, s.depth, h->sparse.depth);
}

void log_distinct_suffixes(const SparseBuildReport &rep, int from, int to) {
    std::fprintf(stderr, "[msbwt] sparse table: distinct suffixes by length:");
    for (int d = from; d <= to; ++d)
        if (rep.distinct[d]) std::fprintf(stderr, " %d: %llu (%llu wide, %llu once)", d, (unsigned long long)rep.distinct[d], (unsigned long long)rep.escapes[d], (unsigned long long)rep.singles[d]);
    std::fprintf(stderr, "\n");
}

// checks, sizing pass, choose, fill -- and maybe choose and fill the second level
int build_sparse(msbwt_rle *h, uint64_t keep_free, uint64_t allowance, int direct_depth, int deep_direct_depth = 0) {
    release_sparse(h);
    const bool explicit_depth = h->wanted_sparse > 0;
    const void *flat = (h->table.entries && !h->table.packed) ? h->table.entries : nullptr;
    const int flat_depth = flat ? h->table.depth : 0;
    const int max_depth = explicit_depth ? h->wanted_sparse : sparse_auto_max_depth(h->query_length);
    if (max_depth <= flat_depth || max_depth < kSparseMinDepth) return explicit_depth ? fail(h, MSBWT_ERR_INVALID_ARG, "sparse table depth must exceed the direct table's") : MSBWT_OK;
    // (the two-tier form sends the suffixes that occur once down the direct table's path: it needs that table's side array for escape lines)
    const int tiers = h->wanted_table_side == 0 ? 0 : h->wanted_tiers;
    if (explicit_depth && tiers == 1 && max_depth <= kTierMaxDepth && !sparse_tier_fits_direct(max_depth, direct_depth))
        return fail(h, MSBWT_ERR_INVALID_ARG, "a two-tier sparse table of depth " + std::to_string(max_depth) + " needs a direct table shallower than it (the direct table is " +
                                                  std::to_string(direct_depth) + " deep)");
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return MSBWT_OK;
    // MSBWT_SPARSE_FRONTIER=<nodes>: (tests) caps the builder's frontier buffers, so that a toy index meets the walker's chunks, retries and descents
    const char *frontier = std::getenv("MSBWT_SPARSE_FRONTIER");
    const size_t work_bytes = sparse_work_bytes(h->totals.total, free_b, frontier ? std::strtoull(frontier, nullptr, 10) : 0);
    auto optional = [&](hipError_t e, const char *what) -> int {  // an optional structure gives way; an explicit wish does not
        (void)hipGetLastError();
        if (explicit_depth) return hip_fail(h, e, what);
        if (verbose()) std::fprintf(stderr, "[msbwt] sparse table: %s: %s -- none built\n", what, hipGetErrorString(e));
        return MSBWT_OK;
    };
    DeviceBuf work, counts;  // both stay allocated until this function returns: the second level is sized beside them
    hipError_t e = work.alloc(work_bytes);
    // (the frontiers start out as zeros, not as whatever the allocation held: a node {0, 0, 0} is harmless wherever it is read)
    if (e == hipSuccess) e = hipMemsetAsync(work.get(), 0, work_bytes, h->stream);
    if (e != hipSuccess) return optional(e, "scratch");
    SparseBuildReport rep;
    e = sparse_count_levels(view_of(h), flat, flat_depth, max_depth, work.get(), work_bytes, &rep, h->stream);
    if (e != hipSuccess) return optional(e, "sizing pass");
    if (verbose()) log_distinct_suffixes(rep, flat_depth, max_depth);
    // (an explicit depth wins over a memory budget, like the other explicit settings: only the HBM itself limits it)
    const uint64_t avail = std::min<uint64_t>(explicit_depth ? kNoBudget : allowance, free_beyond_reserve(keep_free));
    // the depth: a pure function of the counts and the bytes (sparse_policy.hpp, pinned by a CPU test through msbwt_auto_sparse_depth)
    const SparseChoice choice = choose_sparse_depth(rep.distinct, rep.escapes, flat_depth, max_depth, avail, explicit_depth ? max_depth : 0, rep.singles, tiers, direct_depth);
    if (!choice.depth && explicit_depth) return fail(h, MSBWT_ERR_HIP, "the sparse table of the requested depth does not fit in HBM");
    if (!choice.depth) {
        h->sparse_report = rep;  // (the distinct counts are worth keeping: msbwt_rle_sparse_table_info)
        if (verbose()) std::fprintf(stderr, "[msbwt] sparse table: no depth fits %.2f GB -- none built\n", double(avail) / 1e9);
        return MSBWT_OK;
    }
    const SparseWork w{flat, flat_depth, work.get(), work_bytes};
    const char *what = "";
    e = fill_sparse_level(h, w, choice, &rep, 4, avail, &counts, &h->sparse, &what);
    if (e != hipSuccess) return optional(e, what);
    h->sparse_report = rep;
    if (verbose())
        std::fprintf(stderr, "[msbwt] sparse table: depth %d%s, %llu entries in %u buckets (%.2f per bucket, %llu displaced, %llu in the side array, %llu in the filters), %.2f GB; "
                             "chunks / retries / descents: sizing %llu / %llu / %llu, fill %llu / %llu / %llu\n",
                     choice.depth, choice.tier ? " two-tier" : "", (unsigned long long)rep.entries, h->sparse.nbuckets, double(rep.entries) / double(h->sparse.nbuckets),
                     (unsigned long long)rep.displaced, (unsigned long long)rep.nescapes, (unsigned long long)rep.filtered, double(h->sparse.bytes + h->sparse.side_bytes) / 1e9,
                     (unsigned long long)rep.sizing_walk[0], (unsigned long long)rep.sizing_walk[1], (unsigned long long)rep.sizing_walk[2],
                     (unsigned long long)rep.fill_walk[0], (unsigned long long)rep.fill_walk[1], (unsigned long long)rep.fill_walk[2]);
    build_second_sparse_level(h, w, rep, tiers, direct_depth, deep_direct_depth, keep_free, allowance);
    return MSBWT_OK;
}

// Direct table beside a sparse one: only queries shorter than the sparse table's entries (and those with '$' / 'N' among their last
// symbols) still read it, so it stays small -- packed depth 15 (4.6 GB) at most.
constexpr int kDirectDepthBesideSparse = 13;  // levels of the flat table (the packed one: + 2)

// The building half of the pair index (rebuild_pair_index is the policy): pair blocks and superblock table at `stride`, from the plane
// blocks in HBM.  On failure the handle has no pair index.
hipError_t build_pair_blocks(msbwt_rle *h, int stride) {
    PairIndex &p = h->pair;
    const PairIndexSizes sz = pair_index_sizes(h->nblocks, stride);
    DeviceBuf scratch;
    hipError_t e = hipMalloc(&p.blocks, sz.pair_block_bytes);
    if (e == hipSuccess) e = hipMalloc(&p.super, sz.super_bytes);
    if (e == hipSuccess) e = scratch.alloc(sz.scratch_bytes);
    if (e == hipSuccess) e = build_pair_index(h->d_blocks, h->nblocks, h->totals.start_index, p.blocks, p.super, scratch.get(), h->stream, stride);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        p.release();
        return e;
    }
    p.stride = stride;
    p.bytes = sz.pair_block_bytes + sz.super_bytes;
    return hipSuccess;
}

// Run blocks with a sparse table (round 6): the table is built while the PLANE blocks of the load are still in HBM -- temporary pair blocks
// (stride 128) and a flat parent table beside them, then the usual sizing and fill passes -- and only the table stays: pair blocks and
// parent are freed again before the planes become run blocks.  Optional: whatever does not fit leaves the index without a sparse table.
// The caller has made the handle look like a plane-block index (d_blocks = planes, totals, nblocks).
int build_sparse_for_runs(msbwt_rle *h) {
    if (h->wanted_sparse == 0 || h->totals.total == 0) return MSBWT_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return MSBWT_OK;
    const PairIndexSizes sz = pair_index_sizes(h->nblocks, 128);
    // what the conversion will need beside the planes: the run blocks and their overflow blocks -- counted from the planes, as the conversion does
    const uint64_t run_bytes = run_block_count(h->totals.total) * kBlockBytes;
    uint64_t run_peak = run_bytes + run_bytes / 8;
    unsigned long long nover = 0;
    if (count_overflow_blocks(h, h->d_blocks, h->nblocks, h->totals.total, &nover) == hipSuccess) run_peak = run_bytes + uint64_t(nover) * 256;
    else (void)hipGetLastError();
    const int parent = std::min(kDirectDepthBesideSparse, std::max(0, auto_flat_table_depth(h->totals.total, h->nblocks * kBlockBytes)));
    const uint64_t parent_bytes = parent > 0 ? (uint64_t(1) << (2 * parent)) * 16 : 0;
    if (sz.pair_block_bytes + sz.super_bytes + sz.scratch_bytes + parent_bytes + run_peak > uint64_t(free_b) - uint64_t(free_b) / 32) {
        if (verbose()) std::fprintf(stderr, "[msbwt] run blocks: no room for the temporary pair blocks of a sparse-table build -- none built\n");
        return h->wanted_sparse > 0 ? fail(h, MSBWT_ERR_HIP, "the sparse table of the requested depth cannot be built: no room for its temporary pair blocks") : MSBWT_OK;
    }
    auto drop_temps = [&]() {
        h->table.release();
        h->pair.release();
        h->pair.stride = 128;
    };
    hipError_t e = build_pair_blocks(h, 128);
    if (e != hipSuccess) {
        drop_temps();
        (void)hipGetLastError();
        return h->wanted_sparse > 0 ? hip_fail(h, e, "build pair index") : MSBWT_OK;
    }
    if (parent > 0 && build_flat_table(h, parent, &h->table) != hipSuccess) (void)hipGetLastError();  // (no parent: the expansion starts from the root)
    // what the budget leaves once the run blocks and their (flat) direct table are paid for; the conversion's peak stays free.  Run blocks
    // are the memory-LEAN format: left to itself the table (with its build scratch) may take twice what the finished blocks take and no more
    // (human scale: 26.8 GB of run blocks -> 53.6 GB: the depth-23 table, 42 GB, or for a declared k = 31 the depth-27 one, 49 GB; a 3e7-symbol
    // stream, whose depth-23 table the tags would force to 4.3 GB: none) -- an explicit depth or a memory budget says otherwise.
    const uint64_t allowance = h->memory_budget ? budget_left(h, run_peak + parent_bytes) : h->wanted_sparse < 0 ? 2 * run_peak : kNoBudget;
    // (the run blocks' direct table is rebuilt flat afterwards: at most `parent` deep when automatic)
    int rc = build_sparse(h, run_peak, allowance, h->wanted_table_depth >= 0 ? h->wanted_table_depth : parent);
    drop_temps();
    if (rc && h->wanted_sparse <= 0) {
        release_sparse(h);
        h->err.clear();
        rc = MSBWT_OK;
    }
    return rc;
}

// How wide is the range of a k-mer that occurs?  (kernels.hpp, launch_probe_widths: the median over a few thousand
// sampled 24-mers; -1 when it cannot be told.)  Cheap: microseconds of kernel time, one 32 KiB read-back.
double probe_typical_width(msbwt_rle *h) {
    if (h->block_format != kBlocksPlanes || h->totals.total == 0) return -1.0;
    DeviceBuf d_out;
    std::vector<uint64_t> widths(kProbeSamples);
    hipError_t e = d_out.alloc(widths.size() * sizeof(uint64_t));
    if (e == hipSuccess) e = launch_probe_widths(view_of(h), kProbeSamples, kProbeSteps, 0x6D73627774ull, static_cast<uint64_t *>(d_out.get()), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(widths.data(), d_out.get(), widths.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return -1.0;
    }
    widths.erase(std::remove(widths.begin(), widths.end(), uint64_t(0)), widths.end());  // walks that met '$' / 'N'
    if (widths.size() < 64) return -1.0;
    std::nth_element(widths.begin(), widths.begin() + widths.size() / 2, widths.end());
    return double(widths[widths.size() / 2]);
}

// Index build on the host (kept for MSBWT_BUILD=host and for cross-checking the device
// builder): expand into pinned memory, upload.
int build_on_host(msbwt_rle *h, const uint8_t *rle, size_t n, Totals *t_out) {
    Totals t;
    if (int rc = host_totals(h, rle, n, &t)) return rc;
    const uint64_t nblocks = plane_block_count(t.total);
    const size_t bytes = size_t(nblocks) * kBlockBytes;
    uint32_t *host = nullptr;
    // pinned staging so the upload runs at PCIe rate; fall back to pageable memory
    const bool pinned = hipHostMalloc(reinterpret_cast<void **>(&host), bytes, hipHostMallocDefault) == hipSuccess;
    if (!pinned) {
        host = static_cast<uint32_t *>(std::malloc(bytes));
        if (!host) return fail(h, MSBWT_ERR_IO, "out of host memory while building the index");
    }
    build_plane_blocks(rle, n, t, host, 0);
    hipError_t e = hipMalloc(&h->d_blocks, bytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_blocks, host, bytes, hipMemcpyHostToDevice);
    if (pinned) (void)hipHostFree(host);
    else std::free(host);
    if (e != hipSuccess) return hip_fail(h, e, "upload index");
    *t_out = t;
    return MSBWT_OK;
}

// Index build on the device (default): upload the RLE bytes, expand them in HBM
// (device_build.hip).  The expanded index (0.5 B/symbol) never exists on the host.
constexpr int kBuildOnHostInstead = 1000;  // (internal) the run-block path's planes do not fit beside its runs: nothing is left allocated

int build_on_device(msbwt_rle *h, const uint8_t *rle, size_t n, Totals *t_out, bool for_run_blocks = false) {
    DeviceBuf d_rle, scratch, longs;
    HIP_TRY(h, d_rle.alloc(n + 32));
    if (n) HIP_TRY(h, hipMemcpyAsync(d_rle.get(), rle, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, scratch.alloc(device_build_scratch_bytes(n)));
    DeviceBuildState st;
    HIP_TRY(h, device_build_pass1(static_cast<const uint8_t *>(d_rle.get()), n, scratch.get(), &st, h->stream));
    uint64_t head[32];  // totals[7], start_index[6], flags, long_count, ...
    HIP_TRY(h, hipMemcpyAsync(head, scratch.get(), sizeof head, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint32_t flags = *reinterpret_cast<const uint32_t *>(&head[13]);
    const uint64_t nlong = head[15];
    if (flags & kRleBadSymbol) return fail(h, MSBWT_ERR_INVALID_SYMBOL, "RLE stream holds a symbol code >= 6");
    Totals t{};
    uint64_t acc = 0;
    for (int s = 0; s < kAlphabet; ++s) {
        t.symbol_counts[s] = head[s];
        t.start_index[s] = acc;
        acc += head[s];
        t.end_index[s] = acc;
    }
    t.total = acc;
    if ((flags & kRleTooLarge) || t.total >= kMaxSymbols || acc != head[6])
        return fail(h, MSBWT_ERR_TOO_LARGE, "BWT has 2^40 symbols or more");
    const uint64_t nblocks = plane_block_count(t.total);
    const size_t bytes = size_t(nblocks) * kBlockBytes;
    if (for_run_blocks) {  // planes AND runs must fit (table_policy.hpp); MSBWT_RUN_BUILD_FREE=<bytes>: tests pretend that much is free
        size_t free_b = 0, total_b = 0;
        uint64_t free_now = (hipMemGetInfo(&free_b, &total_b) == hipSuccess) ? uint64_t(free_b) : ~uint64_t(0);
        if (const char *env = std::getenv("MSBWT_RUN_BUILD_FREE")) free_now = std::strtoull(env, nullptr, 10);
        if (!run_build_fits_device(t.total, free_now)) return kBuildOnHostInstead;
    }
    {
        const hipError_t e = hipMalloc(&h->d_blocks, bytes);
        if (e == hipErrorOutOfMemory && for_run_blocks) {
            (void)hipGetLastError();
            h->d_blocks = nullptr;
            return kBuildOnHostInstead;
        }
        if (e != hipSuccess) return hip_fail(h, e, "hipMalloc(plane blocks)");
    }
    HIP_TRY(h, hipMemsetAsync(h->d_blocks, 0, bytes, h->stream));
    HIP_TRY(h, hipMemcpyAsync(st.d_start_index, t.start_index, sizeof t.start_index, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, longs.alloc(device_build_long_run_bytes(nlong)));
    HIP_TRY(h, device_build_pass2(static_cast<const uint8_t *>(d_rle.get()), n, st, longs.get(), nlong, h->d_blocks, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *t_out = t;
    return MSBWT_OK;
}

// Run blocks (the memory-lean format, run_index.hpp).  Default (round 4): on the device -- the RLE bytes are expanded into
// plane blocks as for the default format, every run block is made from its two plane blocks (run_build.hip), and the plane
// blocks are freed: 73 GB for a moment instead of 28 GB at human scale, seconds instead of half a minute.  MSBWT_BUILD=host:
// built on the host and uploaded.
// The device half: the plane blocks in h->d_blocks become run blocks (and overflow blocks) there; the planes are gone either way, and
// after a failure so is whatever was made of them.
hipError_t run_blocks_from_planes(msbwt_rle *h, uint64_t total) {
    DeviceBuf planes(h->d_blocks);
    h->d_blocks = nullptr;
    const uint64_t nplanes = plane_block_count(total), nruns = run_block_count(total);
    unsigned long long nover = 0;
    hipError_t e = count_overflow_blocks(h, planes.get(), nplanes, total, &nover);
    if (e == hipSuccess) e = hipMalloc(&h->d_blocks, size_t(nruns) * kBlockBytes);
    if (e == hipSuccess && nover) {
        h->overflow_bytes = uint64_t(nover) * 256;
        e = hipMalloc(&h->d_overflow, h->overflow_bytes);
    }
    if (e == hipSuccess) e = launch_run_block_write(planes.get(), nplanes, total, pack_scratch(h), h->d_blocks, h->d_overflow, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) return e;
    if (h->d_blocks) (void)hipFree(h->d_blocks);
    if (h->d_overflow) (void)hipFree(h->d_overflow);
    h->d_blocks = h->d_overflow = nullptr;
    h->overflow_bytes = 0;
    return e;
}

// The host half: run blocks built on the host and uploaded.
int build_runs_on_host(msbwt_rle *h, const uint8_t *rle, size_t n, Totals *t_out) {
    Totals t;
    if (int rc = host_totals(h, rle, n, &t)) return rc;
    RunIndex ri;
    build_run_blocks(rle, n, t, &ri, 0);
    HIP_TRY(h, hipMalloc(&h->d_blocks, ri.blocks.size() * sizeof(uint32_t)));
    HIP_TRY(h, hipMemcpy(h->d_blocks, ri.blocks.data(), ri.blocks.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!ri.overflow.empty()) {
        h->overflow_bytes = ri.overflow.size() * sizeof(uint32_t);
        HIP_TRY(h, hipMalloc(&h->d_overflow, h->overflow_bytes));
        HIP_TRY(h, hipMemcpy(h->d_overflow, ri.overflow.data(), h->overflow_bytes, hipMemcpyHostToDevice));
    }
    *t_out = t;
    return MSBWT_OK;
}

// The driver.  The device path holds the plane blocks (0.5 byte per symbol), the RLE bytes and its scratch for a moment, and then the run
// blocks beside the planes: about 0.8 byte per symbol at its peak against 0.3 for the finished index.  An index whose planes do
// not fit beside its runs is built on the host instead (as until round 3) -- decided beforehand from the free HBM where the totals
// can be told (run_build_fits_device), and again on the way should an allocation fail after all.
int build_run_index(msbwt_rle *h, const uint8_t *rle, size_t n, Totals *t_out) {
    if (build_on_host_wanted()) return build_runs_on_host(h, rle, n, t_out);
    int rc = build_on_device(h, rle, n, t_out, true);  // h->d_blocks = plane blocks
    if (rc == kBuildOnHostInstead) {
        if (verbose()) std::fprintf(stderr, "[msbwt] run blocks: the device builder's peak does not fit the free HBM -- built on the host\n");
        return build_runs_on_host(h, rle, n, t_out);
    }
    if (rc) return rc;
    if (h->wanted_sparse != 0) {  // (the planes are in h->d_blocks: the handle looks like a plane-block index for a moment)
        h->block_format = kBlocksPlanes;
        h->totals = *t_out;
        h->nblocks = plane_block_count(t_out->total);
        rc = build_sparse_for_runs(h);
        h->block_format = kBlocksRuns;
        if (rc) return rc;
    }
    const hipError_t e = run_blocks_from_planes(h, t_out->total);
    if (e == hipSuccess) return MSBWT_OK;
    if (e != hipErrorOutOfMemory) return hip_fail(h, e, "build run blocks on the device");
    (void)hipGetLastError();  // no room for the run blocks beside the planes: the planes are gone now, the host builder takes over
    if (verbose()) std::fprintf(stderr, "[msbwt] run blocks: out of memory on the device path -- built on the host\n");
    return build_runs_on_host(h, rle, n, t_out);
}

// The depths of the direct table: plain data, decided in one place.  depth: levels of the flat table that is built first (0 or less: none);
// pack: ... and packed into a table two levels deeper; capped: held at kDirectDepthBesideSparse because a sparse table is tried, down from
// uncapped_depth.
struct DirectDepths { int depth; bool pack, capped; int uncapped_depth; };

DirectDepths choose_direct_depths(const msbwt_rle *h, bool try_sparse) {
    // Automatic depths come from ONE decision (table_policy.hpp, pinned by a CPU test through
    // msbwt_auto_table_depths): beside a pair index the flat table is built as deep as the packed one needs.
    const bool automatic = h->wanted_table_depth < 0, paired = h->pair.blocks != nullptr;
    DirectDepths d{h->wanted_table_depth, paired && h->wanted_table_packed > 0, false, 0};  // an explicit depth is packed only on request
    if (automatic && h->planned) {  // a memory budget is in force: the plan has sized the table (table_policy.hpp, plan_index)
        d.depth = h->plan.flat;
        d.pack = h->plan.packed != 0 && paired && h->wanted_table_packed != 0;
    } else if (automatic) {
        size_t free_b = 0, total_b = 0;
        const bool know_free = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        // the table budgets against DISJOINT pair blocks: what overlapping ones take on top was checked against the
        // reserve when they were chosen (choose_pair_stride)
        const TableChoice c = choose_table_depths(h->totals.total, h->nblocks * kBlockBytes, know_free ? uint64_t(free_b) + h->pair.overlap_bytes : 0, paired, h->wanted_table_packed != 0);
        d.depth = c.flat;
        d.pack = c.packed != 0 || (paired && h->wanted_table_packed > 0);  // mode 1: whenever a pair index exists
    }
    d.uncapped_depth = d.depth;
    // The sparse table (sparse_table.hpp) is tried whenever a pair index exists; the automatic direct table then stays small.
    if (try_sparse && automatic && d.depth > kDirectDepthBesideSparse) {
        d.depth = kDirectDepthBesideSparse;
        d.capped = true;
    }
    // (run blocks behind a sparse table -- built at load time, build_sparse_for_runs: the lean format keeps its flat direct table at depth 13,
    // 1 GB instead of 17, for the queries the sparse table does not serve)
    if (h->block_format == kBlocksRuns && h->sparse.lines && automatic && d.depth > kDirectDepthBesideSparse) d.depth = kDirectDepthBesideSparse;
    if (d.depth + 2 > 18) d.pack = false;
    return d;
}

// the handle's flat direct table and the presence filter made from it; a kernel set without a table leaves the handle without one
int build_direct_flat(msbwt_rle *h, int depth) {
    const hipError_t e = build_flat_table(h, depth, &h->table);
    if (e == hipErrorNotSupported) return MSBWT_OK;  // kernel set without a table
    if (e != hipSuccess) return hip_fail(h, e, "build suffix table");
    return rebuild_filter(h);  // from the flat table, before it may be packed away
}

// Packed form, two levels deeper (kernels.hpp, launch_pack_table): every level removes a line fetch
// per query, and the first step after a shallow table is the expensive one (wide ranges straddle
// blocks).  Needs the pair index.  Two passes; the flat table of `depth` levels in the handle is replaced -- or, when packing is optional
// and fails, kept or rebuilt within its own budget.
int pack_direct_table(msbwt_rle *h, int depth) {
    DirectTable &t = h->table;
    const uint64_t pbytes = packed_table_bytes(depth + 2);
    DeviceBuf packed, side;
    unsigned long long *d_cnt = pack_scratch(h);  // [0] escape lines, [1] side cursor
    unsigned long long escapes = 0;
    hipError_t e = packed.alloc(pbytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, 16, h->stream);
    if (e == hipSuccess) e = launch_pack_table(view_of(h), depth, t.entries, packed.get(), d_cnt, nullptr, nullptr, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&escapes, d_cnt, sizeof escapes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    // Escape lines (some delta beyond 16 bits: the suffixes of high-copy repeats) get their ranges as flat entries in a side
    // array, 512 bytes per line, filled by a second pass over those lines only.  Optional: without it (no memory, or
    // MSBWT_TABLE_SIDE=0) their queries search from scratch.
    if (e == hipSuccess && escapes > 0 && h->wanted_table_side != 0) {
        if (side.alloc(size_t(escapes) * 512) != hipSuccess) {
            (void)hipGetLastError();
        } else {
            e = launch_pack_table(view_of(h), depth, t.entries, packed.get(), nullptr, side.get(), d_cnt + 1, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
    }
    if (e != hipSuccess) {
        side.reset();
        packed.reset();
        (void)hipGetLastError();
        if (h->wanted_table_depth >= 0 || h->wanted_table_packed > 0) return hip_fail(h, e, "pack suffix table");
        // optional structure: the handle keeps a flat table -- within the flat table's OWN budget, not the
        // deeper parent that was only meant to be packed away
        const int own = auto_flat_table_depth(h->totals.total, h->nblocks * kBlockBytes);
        if (own >= depth) return MSBWT_OK;
        t.release();
        return own > 0 ? build_direct_flat(h, own) : MSBWT_OK;
    }
    DeviceBuf flat(t.entries);  // the flat table goes
    t.entries = packed.release();
    t.depth = depth + 2;
    t.packed = true;
    t.bytes = pbytes;
    t.side = side.release();
    t.side_bytes = t.side ? uint64_t(escapes) * 512 : 0;
    t.lines = pbytes / 128;
    t.escape_lines = escapes;
    return MSBWT_OK;
}

constexpr int kAgainWithoutSparse = 1001;  // (internal) build_tables: the tables are to be built as if there were no sparse table

// The two-tier table sends queries down the packed direct table's path, and an escape line without its side entry cannot be followed from
// there (the query's first symbols are gone): no room for the side array -> the index as if there were no sparse table -- unless
// that very table was asked for, which is then an error (as an explicit depth that does not fit).
int check_tiers_have_side_array(msbwt_rle *h) {
    if (h->table.escape_lines == 0 || h->table.side) return MSBWT_OK;
    if (h->sparse2.lines && h->sparse2.tier && !h->sparse.tier) h->sparse2.release();  // (only the second level is two-tier: it alone goes)
    if (!h->sparse.lines || !(h->sparse.tier || h->sparse2.tier)) return MSBWT_OK;
    if (h->wanted_sparse > 0 && h->wanted_tiers == 1 && h->sparse.tier) {
        release_sparse(h);
        return fail(h, MSBWT_ERR_HIP, "the two-tier sparse table of the requested depth cannot be kept: no room for the direct table's side array");
    }
    return kAgainWithoutSparse;
}

// Direct table, filter, sparse table(s) and packed form of a loaded index, in that order.  kAgainWithoutSparse: a sparse table was tried
// and the index is better off without (rebuild_table calls again with try_sparse = false).
int build_tables(msbwt_rle *h, bool try_sparse) {
    // (run blocks: their sparse table was built at load time from temporary plane and pair blocks -- build_sparse_for_runs -- and does
    // not depend on the direct table rebuilt here; it goes with the index, or by msbwt_rle_set_sparse_table(0))
    if (h->block_format == kBlocksPlanes) release_sparse(h);
    DirectTable &t = h->table;
    t.release();
    DirectDepths d = choose_direct_depths(h, try_sparse);
    if (d.depth <= 0 && !try_sparse) return MSBWT_OK;
    int rc = d.depth > 0 ? build_direct_flat(h, d.depth) : MSBWT_OK;
    if (rc) return rc;
    if (try_sparse) {
        const uint64_t packed_later = (d.pack && t.entries) ? packed_table_bytes(d.depth + 2) : 0;
        // what the budget leaves once blocks, pair blocks and the direct table are paid for
        const uint64_t allowance = h->planned ? budget_left(h, h->nblocks * kBlockBytes + h->pair.bytes + (packed_later ? packed_later : uint64_t(t.bytes))) : kNoBudget;
        rc = build_sparse(h, packed_later, allowance, t.entries ? d.depth + (d.pack ? 2 : 0) : 0, (d.capped && d.pack) ? d.uncapped_depth : 0);
        if (rc) return rc;
        // Should no sparse depth fit (a read set whose error k-mers outnumber the genome's many times over), the direct table is built
        // again as if there were no such thing.
        if (!h->sparse.lines && d.capped) return kAgainWithoutSparse;
    }
    // Beside a sparse table the direct table serves the queries SHORTER than that table's entries (and those with '$' / 'N' among their
    // last symbols).  Capped at packed depth 15 those lose against the index without a sparse table (round 6, human scale, present
    // k-mers: k = 17 2.5 x, k = 19 1.8 x, k = 21 1.5 x slower than behind the packed depth-17 table) -- so where HBM is plentiful (a
    // chr20-sized index: 15 GB of 288) the deep direct table is kept AS WELL: nothing is lost for any k.  Not under a memory budget
    // (the plan has sized the table), and not where it would take the eighth of the device left to the caller's batches (deep_direct_fits);
    // there build_sparse has tried a second, shallower sparse level instead.  Nor where a two-tier table would then be no deeper than the
    // direct table its filter sends queries to (sparse_tier_fits_direct: a declared k = 16 or 17).
    if (d.capped && h->sparse.lines && !h->sparse2.lines && t.entries && d.pack && (!h->sparse.tier || sparse_tier_fits_direct(h->sparse.depth, d.uncapped_depth + 2)) &&
        deep_direct_fits(h, d.uncapped_depth)) {
        t.release();
        d.depth = d.uncapped_depth;
        rc = build_direct_flat(h, d.depth);
        if (rc) return rc;
    }
    if (!t.entries || !d.pack) return rc;
    rc = pack_direct_table(h, d.depth);
    return (rc || !t.packed) ? rc : check_tiers_have_side_array(h);
}

// A memory budget (msbwt_rle_set_memory_budget) turns the automatic choices into ONE plan, made once the plane blocks are in
// HBM and the data have been probed (table_policy.hpp, plan_index: pair blocks, then the deepest packed table, then
// overlapping pair blocks).  Run blocks have no optional structures but the flat table.
void make_plan(msbwt_rle *h) {
    h->planned = false;
    if (h->memory_budget == 0 || h->block_format != kBlocksPlanes) return;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    const PairIndexSizes wide = pair_index_sizes(h->nblocks, 96), narrow = pair_index_sizes(h->nblocks, 128);
    h->plan = plan_index(h->totals.total, free_b, total_b, h->typical_width, h->memory_budget, narrow.pair_block_bytes + narrow.super_bytes,
                         wide.pair_block_bytes + wide.super_bytes);
    h->planned = true;
}

// Pair index (two symbols per step, rank_ops.hpp): 1 byte/symbol on top of the plane blocks,
// built on the device from them.  Default policy: build it when it fits in half of what is
// still free in HBM after the blocks (it is a pure speed-for-memory trade).
// The policy half: whether to build, at which stride, and whether the data chose it; build_pair_blocks does the building.
int rebuild_pair_index(msbwt_rle *h) {
    PairIndex &p = h->pair;
    p.release();
    if (h->wanted_pair == 0 || h->totals.total == 0 || h->block_format != kBlocksPlanes) return MSBWT_OK;  // built from plane blocks
    // Spacing (table_policy.hpp, choose_pair_stride): an explicit wish is taken literally; otherwise overlapping
    // blocks (stride 96, 1.33 bytes per symbol: ranges up to 32 wide from one line) when they are cheap in HBM, and
    // when they are not, when the DATA keep the ranges of present k-mers wide (probed above) and the bigger blocks
    // fit beside the table that is about to be built.
    size_t free_b = 0, total_b = 0;
    const bool know_free = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    int stride = h->wanted_pair_stride;
    bool by_data = false;
    if (h->planned && h->wanted_pair < 0 && !h->plan.pair) return MSBWT_OK;  // the memory budget has no room for pair blocks
    if (h->planned && stride != 96 && stride != 128) {
        stride = h->plan.stride;
        by_data = true;  // (the plan has checked the fit)
    } else if (stride != 96 && stride != 128) {
        const PairIndexSizes wide = pair_index_sizes(h->nblocks, 96), narrow = pair_index_sizes(h->nblocks, 128);
        const uint64_t bytes96 = wide.pair_block_bytes + wide.super_bytes + wide.scratch_bytes, bytes128 = narrow.pair_block_bytes + narrow.super_bytes;
        const uint64_t after128 = uint64_t(free_b) > bytes128 ? uint64_t(free_b) - bytes128 : 0;
        const uint64_t table_b = expected_table_bytes(h->totals.total, h->nblocks * kBlockBytes, after128, true, h->wanted_table_packed != 0);
        stride = know_free ? choose_pair_stride(bytes96, table_b, free_b, total_b, h->typical_width) : 128;
        by_data = stride == 96 && bytes96 > uint64_t(free_b) / 4;
        if (by_data) p.overlap_bytes = wide.pair_block_bytes + wide.super_bytes - bytes128;
    }
    const PairIndexSizes sz = pair_index_sizes(h->nblocks, stride);
    if (h->wanted_pair < 0 && !by_data) {  // (the data-driven choice has checked its own fit)
        if (!know_free || sz.pair_block_bytes + sz.scratch_bytes > free_b / 2) return MSBWT_OK;
    }
    const hipError_t e = build_pair_blocks(h, stride);
    if (e == hipSuccess || (h->wanted_pair < 0 && e == hipErrorOutOfMemory)) return MSBWT_OK;  // optional structure
    return hip_fail(h, e, "build pair index");
}

}  // namespace

namespace msbwt_capi {

// both sparse levels and what the sizing pass counted
void release_sparse(msbwt_rle *h) {
    h->sparse.release();
    h->sparse_report = SparseBuildReport{};
    h->sparse2.release();
}

void release_index(msbwt_rle *h) {
    if (h->d_blocks) (void)hipFree(h->d_blocks);
    if (h->d_overflow) (void)hipFree(h->d_overflow);
    h->d_blocks = h->d_overflow = nullptr;
    h->overflow_bytes = 0;
    h->table.release();
    release_sparse(h);
    h->pair.release();
    h->sources.release();  // the colouring is of the rows that go
    h->nblocks = 0;
    h->typical_width = -1.0;
    h->totals = Totals{};  // an unloaded handle reports 0 symbols, not the previous BWT's
    h->loaded = false;
}

// The tables of a loaded index, rebuilt by the handle's settings.  A sparse table is tried whenever a pair index exists; where the index
// turns out better off without one (no depth fits; a two-tier level without the direct table's side array) the tables are built once
// more as if there were no such thing -- the distinct counts of the sizing pass stay on record.
int rebuild_table(msbwt_rle *h) {
    const bool try_sparse = h->wanted_sparse != 0 && h->pair.blocks != nullptr && h->block_format == kBlocksPlanes && h->totals.total > 0;
    int rc = build_tables(h, try_sparse);
    if (rc != kAgainWithoutSparse) return rc;
    const SparseBuildReport counted = h->sparse_report;
    rc = build_tables(h, false);
    h->sparse_report = counted;
    return rc;
}

// the table's packed form exists only beside a pair index: both are rebuilt
int rebuild_pair_and_table(msbwt_rle *h) {
    const int rc = rebuild_pair_index(h);  // first: the table may be packed with its help
    return rc ? rc : rebuild_table(h);
}

// A new memory budget on a loaded index (h->memory_budget == bytes): the optional structures are rebuilt under it (the plan counts the
// memory they hold now as free).  Run blocks: their sparse table was built at load time and cannot be rebuilt (the plane blocks it came
// from are gone) -- it stays while the index fits the budget.
int replan(msbwt_rle *h, uint64_t bytes) {
    if (h->block_format == kBlocksPlanes || (bytes != 0 && msbwt_rle_device_bytes(h) > bytes)) release_sparse(h);
    h->table.release();
    h->pair.release();
    make_plan(h);
    return rebuild_pair_and_table(h);
}

// Common tail of both load entry points: build the blocks in HBM, then the pair index and the table.
// The previous index is released FIRST (two human-scale indexes do not fit one GPU): a failed load
// leaves the handle unloaded -- total size and symbol counts 0, queries MSBWT_ERR_NOT_LOADED.
int install(msbwt_rle *h, const uint8_t *rle, size_t n) {
    DeviceScope scope(h->device);
    if (!scope.ok()) return fail(h, MSBWT_ERR_HIP, scope.why());
    release_index(h);
    int rc = ensure_runtime(h);
    if (rc) return rc;
    // one stderr line per load stage (the reference logs its load milestones with log::info!, rle_bwt.rs:62,149,347,383)
    auto clock = std::chrono::steady_clock::now();
    auto stage = [&](const char *what, uint64_t bytes) {
        if (!verbose()) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[msbwt] load: %-22s %7.2f s  %8.2f GB in HBM\n", what, std::chrono::duration<double>(now - clock).count(), double(bytes) / 1e9);
        clock = now;
    };
    Totals t{};
    h->block_format = h->wanted_block_format;
    if (h->block_format == kBlocksRuns) rc = build_run_index(h, rle, n, &t);
    else rc = build_on_host_wanted() ? build_on_host(h, rle, n, &t) : build_on_device(h, rle, n, &t);
    if (rc) {
        release_index(h);
        return rc;
    }
    h->totals = t;
    h->nblocks = h->block_format == kBlocksRuns ? run_block_count(t.total) : plane_block_count(t.total);
    h->loaded = true;
    stage(h->block_format == kBlocksRuns ? "run blocks" : "plane blocks", h->nblocks * kBlockBytes + h->overflow_bytes);
    h->typical_width = probe_typical_width(h);
    make_plan(h);
    rc = rebuild_pair_index(h);  // first: the table may be packed with its help
    if (!rc) stage(h->pair.stride == 96 ? "pair blocks, stride 96" : "pair blocks, stride 128", h->pair.bytes);
    if (!rc) rc = rebuild_table(h);
    if (!rc) stage(h->table.packed ? "suffix table, packed" : "suffix table, flat", h->table.bytes);
    if (!rc && h->sparse.lines) stage("sparse suffix table", h->sparse.bytes + h->sparse.side_bytes);
    if (rc) {
        release_index(h);
        return rc;
    }
    if (verbose())
        std::fprintf(stderr, "[msbwt] load: %llu symbols, table depth %d, a present %u-mer occurs %.0f times (median), %.2f GB of HBM in all\n",
                     (unsigned long long)t.total, h->table.depth, kProbeSteps, h->typical_width,
                     double(h->nblocks * kBlockBytes + h->overflow_bytes + h->pair.bytes + h->table.bytes + h->sparse.bytes + h->sparse.side_bytes) / 1e9);
    if (verbose())  // where the arrays landed (run-to-run differences of up to 15 % on one box follow the process, not the clocks: profiles/r04_lab)
        std::fprintf(stderr, "[msbwt] load: blocks %p pair blocks %p pair super %p table %p side %p filter %p\n", h->d_blocks, h->pair.blocks,
                     h->pair.super, h->table.entries, h->table.side, static_cast<void *>(h->table.filter));
    h->err.clear();
    return MSBWT_OK;
}

}  // namespace msbwt_capi
