// The index loader: plane and run blocks, pair index, direct, packed and sparse tables, and the memory plan -- what sits in HBM and why.
// The other units reach it through index_build.hpp only; it calls the kernels' host launchers and the shared helpers of handle.hpp.
#include "index_build.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_build.hpp"
#include "handle.hpp"
#include "pair_index.hpp"
#include "plane_index.hpp"
#include "run_build.hpp"
#include "run_index.hpp"

namespace {

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
    uint32_t *filter = nullptr;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void **>(&filter), words * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(filter, 0, words * sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = launch_build_filter(t.entries, t.depth, fd, filter, h->stream);
    std::vector<uint32_t> host(words);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), filter, words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipFree(filter);
        return hip_fail(h, e, "build presence filter");
    }
    uint64_t set = 0;
    for (uint32_t w : host) set += uint64_t(__builtin_popcount(w));
    if (double(set) > 0.9 * double(words * 32)) {
        (void)hipFree(filter);
        return MSBWT_OK;
    }
    t.filter = filter;
    t.filter_depth = fd;
    return MSBWT_OK;
}

// Sparse suffix table (sparse_table.hpp) from the flat direct table that is in HBM right now (its parent; none: from the root).
// Optional structure: when nothing fits (or a step fails for want of memory) the handle simply has none -- unless a depth was
// asked for explicitly, which is then an error.  keep_free: bytes that what is built afterwards (the packed direct table) still
// needs; allowance: what a memory budget leaves for this table (kNoBudget: none in force).
// direct_depth: the depth the direct table will have once the sparse table is built (packed: two deeper than the flat one in HBM now; 0 =
// none) -- a two-tier level may not be shallower (sparse_tier_fits_direct).
// deep_direct_depth: the flat depth of the DEEP direct table that is kept beside the sparse table when HBM is plentiful (rebuild_table; 0 =
// not in question) -- where that one fits no second sparse level is built.
constexpr int kSparseSecondDepth = 17;  // entries of the second, shallower level (what the packed direct table of round 4 reached)

bool deep_direct_fits(const msbwt_rle *h, int flat_depth_wanted) {
    if (flat_depth_wanted <= 0 || flat_depth_wanted + 2 > 18 || h->planned) return false;
    size_t free_b = 0, total_b = 0;
    const uint64_t flat_deep = (uint64_t(1) << (2 * flat_depth_wanted)) * 16, packed = packed_table_bytes(flat_depth_wanted + 2);
    const uint64_t need = flat_deep + packed + packed / 8;  // (the packer's side array of escape lines: an eighth at most in practice)
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && uint64_t(free_b) + h->table.bytes >= need + uint64_t(total_b) / 8;
}

int build_sparse(msbwt_rle *h, uint64_t keep_free, uint64_t allowance, int direct_depth, int deep_direct_depth = 0) {
    release_sparse(h);
    const bool verbose = std::getenv("MSBWT_VERBOSE") != nullptr;
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
    struct Temps {
        void *work = nullptr, *counts = nullptr, *lines = nullptr, *side = nullptr;
        ~Temps() {
            for (void *p : {work, counts, lines, side})
                if (p) (void)hipFree(p);
        }
    } tmp;
    // (never more scratch than the index can fill: the nodes of a level are disjoint non-empty ranges, at most `total` of them -- a toy
    // index must not pay for a 6 GB allocation per build)
    const size_t work_bytes = std::min<size_t>(sparse_work_bytes(free_b), 4096 + 2 * 24 * size_t(std::max<uint64_t>(h->totals.total + 1024, 4096)));
    auto optional = [&](hipError_t e, const char *what) -> int {  // an optional structure gives way; an explicit wish does not
        (void)hipGetLastError();
        if (explicit_depth) return hip_fail(h, e, what);
        if (verbose) std::fprintf(stderr, "[msbwt] sparse table: %s: %s -- none built\n", what, hipGetErrorString(e));
        return MSBWT_OK;
    };
    hipError_t e = hipMalloc(&tmp.work, work_bytes);
    if (e != hipSuccess) return optional(e, "scratch");
    // (the frontiers start out as zeros, not as whatever the allocation held: a node {0, 0, 0} is harmless wherever it is read)
    e = hipMemsetAsync(tmp.work, 0, work_bytes, h->stream);
    if (e != hipSuccess) return optional(e, "scratch");
    SparseBuildReport rep;
    e = sparse_count_levels(view_of(h), flat, flat_depth, max_depth, tmp.work, work_bytes, &rep, h->stream);
    if (e != hipSuccess) return optional(e, "sizing pass");
    if (verbose) {
        std::fprintf(stderr, "[msbwt] sparse table: distinct suffixes by length:");
        for (int d = flat_depth; d <= max_depth; ++d)
            if (rep.distinct[d]) std::fprintf(stderr, " %d: %llu (%llu wide, %llu once)", d, (unsigned long long)rep.distinct[d], (unsigned long long)rep.escapes[d], (unsigned long long)rep.singles[d]);
        std::fprintf(stderr, "\n");
    }
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return MSBWT_OK;
    const uint64_t spare = keep_free + total_b / 8;  // an eighth of the HBM stays free for the caller's batches
    // (an explicit depth wins over a memory budget, like the other explicit settings: only the HBM itself limits it)
    const uint64_t avail = std::min<uint64_t>(explicit_depth ? kNoBudget : allowance, uint64_t(free_b) > spare ? uint64_t(free_b) - spare : 0);
    // the depth: a pure function of the counts and the bytes (sparse_policy.hpp, pinned by a CPU test through msbwt_auto_sparse_depth)
    const SparseChoice choice = choose_sparse_depth(rep.distinct, rep.escapes, flat_depth, max_depth, avail, explicit_depth ? max_depth : 0, rep.singles, tiers, direct_depth);
    const int chosen = choice.depth;
    uint64_t nbuckets = choice.nbuckets;
    if (!chosen && explicit_depth) return fail(h, MSBWT_ERR_HIP, "the sparse table of the requested depth does not fit in HBM");
    if (!chosen) {
        h->sparse_report = rep;  // (the distinct counts are worth keeping: msbwt_rle_sparse_table_info)
        if (verbose) std::fprintf(stderr, "[msbwt] sparse table: no depth fits %.2f GB -- none built\n", double(avail) / 1e9);
        return MSBWT_OK;
    }
    const uint64_t nside = rep.escapes[chosen];
    if (nside) {
        e = hipMalloc(&tmp.side, nside * 16);
        if (e != hipSuccess) return optional(e, "side array");
    }
    for (int attempt = 0;; ++attempt) {
        const int probe = sparse_probe_limit(chosen, nbuckets);
        if (probe < 1) return optional(hipErrorInvalidValue, "bucket count");
        const uint64_t lines = nbuckets + uint64_t(probe);
        e = hipMalloc(&tmp.lines, lines * 128);
        if (e == hipSuccess) e = hipMalloc(&tmp.counts, lines * sizeof(uint32_t));
        if (e != hipSuccess) return optional(e, "bucket lines");
        e = sparse_fill(view_of(h), flat, flat_depth, chosen, choice.tier, tmp.lines, nbuckets, uint32_t(probe), tmp.side, nside, tmp.counts, tmp.work, work_bytes, &rep, h->stream);
        if (e == hipSuccess) {
            h->sparse = SparseLevel{tmp.lines, tmp.side, lines * 128, nside * 16, 0, uint32_t(nbuckets), uint32_t(probe), chosen, choice.tier};
            tmp.lines = tmp.side = nullptr;
            break;
        }
        if (e != hipErrorInvalidValue || attempt == 3) return optional(e, "fill pass");
        (void)hipFree(tmp.lines);  // some entry found no slot within the probe limit: a quarter more buckets
        (void)hipFree(tmp.counts);
        tmp.lines = tmp.counts = nullptr;
        nbuckets += nbuckets / 4;
        // the larger table must still fit what the first one was chosen within (the budget, the eighth of HBM left to the caller) and the format
        const uint64_t again = nbuckets + kSparseMaxProbe;
        if (again > 0xFFFFFFFFull || again * 128 + again * sizeof(uint32_t) + nside * 16 > avail) return optional(hipErrorOutOfMemory, "fill pass (no room for more buckets)");
    }
    h->sparse_report = rep;
    if (verbose)
        std::fprintf(stderr, "[msbwt] sparse table: depth %d%s, %llu entries in %u buckets (%.2f per bucket, %llu displaced, %llu in the side array, %llu in the filters), %.2f GB\n", chosen,
                     choice.tier ? " two-tier" : "", (unsigned long long)rep.entries, h->sparse.nbuckets, double(rep.entries) / double(nbuckets), (unsigned long long)rep.displaced,
                     (unsigned long long)rep.nescapes, (unsigned long long)rep.filtered, double(h->sparse.bytes + h->sparse.side_bytes) / 1e9);
    // ---- a second, shallower level for the queries this table is too deep for (sparse_for, kernels.hpp) ----------------------------------
    // With k undeclared the table above is 23 deep and k = 17..22 fall to the direct table, which stays at packed depth 15 beside a sparse
    // table: measured at human scale (round 6, present k-mers), k = 17 / 19 / 21 run 2.5 / 1.8 / 1.5 x slower than on the index WITHOUT a
    // sparse table (packed depth 17).  Where the deep direct table itself fits (rebuild_table keeps it then) nothing is needed; otherwise the
    // same sizing counts and chunk plan fill a table of the suffixes of 17 symbols -- when it fits what is left, an eighth of the device still
    // free.  A declared k gets none (the caller has said what it will ask), an explicit depth neither.
    // (run blocks are the memory-lean format: no second level there)
    if (!explicit_depth && h->wanted_second != 0 && h->wanted_block_format == kBlocksPlanes && h->query_length == 0 && chosen > kSparseSecondDepth &&
        !deep_direct_fits(h, deep_direct_depth) &&
        hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const uint64_t used = h->sparse.bytes + h->sparse.side_bytes;
        const uint64_t avail2 = std::min<uint64_t>(allowance > used ? allowance - used : 0, uint64_t(free_b) > spare ? uint64_t(free_b) - spare : 0);
        const SparseChoice second = choose_sparse_depth(rep.distinct, rep.escapes, flat_depth, std::min(kSparseSecondDepth, chosen - 1), avail2, 0, rep.singles, tiers, direct_depth);
        if (second.depth) {
            Temps two;  // (its own buffers: the first table's are the handle's by now)
            SparseBuildReport rep2 = rep;
            const int probe2 = sparse_probe_limit(second.depth, second.nbuckets);
            const uint64_t lines2 = second.nbuckets + uint64_t(std::max(probe2, 0)), nside2 = rep.escapes[second.depth];
            e = probe2 >= 1 ? hipSuccess : hipErrorInvalidValue;
            if (e == hipSuccess && nside2) e = hipMalloc(&two.side, nside2 * 16);
            if (e == hipSuccess) e = hipMalloc(&two.lines, lines2 * 128);
            if (e == hipSuccess) e = hipMalloc(&two.counts, lines2 * sizeof(uint32_t));
            if (e == hipSuccess)
                e = sparse_fill(view_of(h), flat, flat_depth, second.depth, second.tier, two.lines, second.nbuckets, uint32_t(probe2), two.side, nside2, two.counts, tmp.work, work_bytes, &rep2,
                                h->stream);
            if (e == hipSuccess) {
                h->sparse2 = SparseLevel{two.lines, two.side, lines2 * 128, nside2 * 16, rep2.entries, uint32_t(second.nbuckets),
                                         uint32_t(probe2), second.depth, second.tier};
                two.lines = two.side = nullptr;
                if (verbose)
                    std::fprintf(stderr, "[msbwt] sparse table, second level: depth %d%s, %llu entries in %u buckets, %.2f GB (serves %d <= k < %d)\n", second.depth,
                                 second.tier ? " two-tier" : "", (unsigned long long)rep2.entries, uint32_t(second.nbuckets), double(lines2 * 128 + nside2 * 16) / 1e9,
                                 second.depth, chosen);
            } else {  // optional: an entry without a slot, no memory -- the index simply has no second level
                (void)hipGetLastError();
                if (verbose) std::fprintf(stderr, "[msbwt] sparse table, second level: %s -- none built\n", hipGetErrorString(e));
            }
        }
    }
    return MSBWT_OK;
}

// Direct table beside a sparse one: only queries shorter than the sparse table's entries (and those with '$' / 'N' among their last
// symbols) still read it, so it stays small -- packed depth 15 (4.6 GB) at most.
constexpr int kDirectDepthBesideSparse = 13;  // levels of the flat table (the packed one: + 2)

// Run blocks with a sparse table (round 6): the table is built while the PLANE blocks of the load are still in HBM -- temporary pair blocks
// (stride 128) and a flat parent table beside them, then the usual sizing and fill passes -- and only the table stays: pair blocks and
// parent are freed again before the planes become run blocks.  Optional: whatever does not fit leaves the index without a sparse table.
// The caller has made the handle look like a plane-block index (d_blocks = planes, totals, nblocks).
int build_sparse_for_runs(msbwt_rle *h) {
    const bool verbose = std::getenv("MSBWT_VERBOSE") != nullptr;
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
        if (verbose) std::fprintf(stderr, "[msbwt] run blocks: no room for the temporary pair blocks of a sparse-table build -- none built\n");
        return h->wanted_sparse > 0 ? fail(h, MSBWT_ERR_HIP, "the sparse table of the requested depth cannot be built: no room for its temporary pair blocks") : MSBWT_OK;
    }
    const Settings saved = *h;
    h->wanted_pair = 1;
    h->wanted_pair_stride = 128;
    h->planned = false;
    int rc = rebuild_pair_index(h);
    static_cast<Settings &>(*h) = saved;
    auto drop_temps = [&]() {
        h->table.release();
        h->pair.release();
        h->pair.stride = 128;
    };
    if (rc || !h->pair.blocks) {
        drop_temps();
        (void)hipGetLastError();
        if (h->wanted_sparse > 0) return rc ? rc : fail(h, MSBWT_ERR_HIP, "the sparse table of the requested depth cannot be built: no pair blocks");
        h->err.clear();
        return MSBWT_OK;
    }
    if (parent > 0) {
        void *tab = nullptr;
        hipError_t e = hipMalloc(&tab, parent_bytes);
        if (e == hipSuccess) e = launch_build_table(view_of(h), parent, tab, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            if (tab) (void)hipFree(tab);
            (void)hipGetLastError();
            tab = nullptr;
        }
        h->table.entries = tab;
        h->table.depth = tab ? parent : 0;
        h->table.bytes = tab ? parent_bytes : 0;
        h->table.packed = false;
    }
    // what the budget leaves once the run blocks and their (flat) direct table are paid for; the conversion's peak stays free.  Run blocks
    // are the memory-LEAN format: left to itself the table (with its build scratch) may take twice what the finished blocks take and no more
    // (human scale: 26.8 GB of run blocks -> 53.6 GB: the depth-23 table, 42 GB, or for a declared k = 31 the depth-27 one, 49 GB; a 3e7-symbol
    // stream, whose depth-23 table the tags would force to 4.3 GB: none) -- an explicit depth or a memory budget says otherwise.
    uint64_t allowance = h->wanted_sparse < 0 ? 2 * run_peak : kNoBudget;
    if (h->memory_budget) {
        const uint64_t held = run_peak + parent_bytes;
        allowance = h->memory_budget > held ? h->memory_budget - held : 0;
    }
    // (the run blocks' direct table is rebuilt flat afterwards: at most `parent` deep when automatic)
    rc = build_sparse(h, run_peak, allowance, h->wanted_table_depth >= 0 ? h->wanted_table_depth : parent);
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
    uint64_t *d_out = nullptr;
    std::vector<uint64_t> widths(kProbeSamples);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_out), widths.size() * sizeof(uint64_t));
    if (e == hipSuccess) e = launch_probe_widths(view_of(h), kProbeSamples, kProbeSteps, 0x6D73627774ull, d_out, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(widths.data(), d_out, widths.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (d_out) (void)hipFree(d_out);
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
    if (!compute_totals(rle, n, &t)) return fail(h, MSBWT_ERR_INVALID_SYMBOL, "RLE stream holds a symbol code >= 6");
    if (t.total > kMaxTotal) return fail(h, MSBWT_ERR_TOO_LARGE, "BWT has 2^40 symbols or more");
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
    struct Temps {
        void *rle = nullptr, *scratch = nullptr, *longs = nullptr;
        ~Temps() {
            for (void *p : {rle, scratch, longs})
                if (p) (void)hipFree(p);
        }
    } tmp;
    HIP_TRY(h, hipMalloc(&tmp.rle, n + 32));
    if (n) HIP_TRY(h, hipMemcpyAsync(tmp.rle, rle, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMalloc(&tmp.scratch, device_build_scratch_bytes(n)));
    DeviceBuildState st;
    HIP_TRY(h, device_build_pass1(static_cast<const uint8_t *>(tmp.rle), n, tmp.scratch, &st, h->stream));
    uint64_t head[32];  // totals[7], start_index[6], flags, long_count, ...
    HIP_TRY(h, hipMemcpyAsync(head, tmp.scratch, sizeof head, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint32_t flags = *reinterpret_cast<const uint32_t *>(&head[13]);
    const uint64_t nlong = head[15];
    if (flags & kBuildBadSymbol) return fail(h, MSBWT_ERR_INVALID_SYMBOL, "RLE stream holds a symbol code >= 6");
    Totals t{};
    uint64_t acc = 0;
    for (int s = 0; s < kAlphabet; ++s) {
        t.symbol_counts[s] = head[s];
        t.start_index[s] = acc;
        acc += head[s];
        t.end_index[s] = acc;
    }
    t.total = acc;
    if ((flags & kBuildTooLarge) || t.total > kMaxTotal || acc != head[6])
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
    HIP_TRY(h, hipMalloc(&tmp.longs, device_build_long_run_bytes(nlong)));
    HIP_TRY(h, device_build_pass2(static_cast<const uint8_t *>(tmp.rle), n, st, tmp.longs, nlong, h->d_blocks, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *t_out = t;
    return MSBWT_OK;
}

// Run blocks (the memory-lean format, run_index.hpp).  Default (round 4): on the device -- the RLE bytes are expanded into
// plane blocks as for the default format, every run block is made from its two plane blocks (run_build.hip), and the plane
// blocks are freed: 73 GB for a moment instead of 28 GB at human scale, seconds instead of half a minute.  MSBWT_BUILD=host:
// built on the host and uploaded.
int build_run_index(msbwt_rle *h, const uint8_t *rle, size_t n, Totals *t_out) {
    const char *mode = std::getenv("MSBWT_BUILD");
    auto sparse_while_planes = [&]() -> int {  // (the planes are in h->d_blocks: the handle looks like a plane-block index for a moment)
        if (h->wanted_sparse == 0) return MSBWT_OK;
        h->block_format = kBlocksPlanes;
        h->totals = *t_out;
        h->nblocks = plane_block_count(t_out->total);
        const int rc = build_sparse_for_runs(h);
        h->block_format = kBlocksRuns;
        return rc;
    };
    // The device path holds the plane blocks (0.5 byte per symbol), the RLE bytes and its scratch for a moment, and then the run
    // blocks beside the planes: about 0.8 byte per symbol at its peak against 0.3 for the finished index.  An index whose planes do
    // not fit beside its runs is built on the host instead (as until round 3) -- decided beforehand from the free HBM where the totals
    // can be told (run_build_fits_device), and again on the way should an allocation fail after all.
    bool on_device = !(mode && std::strcmp(mode, "host") == 0);
    if (on_device) {
        int rc = build_on_device(h, rle, n, t_out, true);  // h->d_blocks = plane blocks
        if (rc == kBuildOnHostInstead) {
            if (std::getenv("MSBWT_VERBOSE")) std::fprintf(stderr, "[msbwt] run blocks: the device builder's peak does not fit the free HBM -- built on the host\n");
            on_device = false;
        } else if (rc) {
            return rc;
        }
    }
    if (on_device) {
        const int rcs = sparse_while_planes();
        if (rcs) return rcs;
        void *planes = h->d_blocks;
        h->d_blocks = nullptr;
        const uint64_t nplanes = plane_block_count(t_out->total), nruns = run_block_count(t_out->total);
        unsigned long long nover = 0;
        hipError_t e = count_overflow_blocks(h, planes, nplanes, t_out->total, &nover);
        if (e == hipSuccess) e = hipMalloc(&h->d_blocks, size_t(nruns) * kBlockBytes);
        if (e == hipSuccess && nover) {
            h->overflow_bytes = uint64_t(nover) * 256;
            e = hipMalloc(&h->d_overflow, h->overflow_bytes);
        }
        if (e == hipSuccess) e = launch_run_block_write(planes, nplanes, t_out->total, pack_scratch(h), h->d_blocks, h->d_overflow, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        (void)hipFree(planes);
        if (e == hipSuccess) return MSBWT_OK;
        if (h->d_blocks) (void)hipFree(h->d_blocks);
        if (h->d_overflow) (void)hipFree(h->d_overflow);
        h->d_blocks = h->d_overflow = nullptr;
        h->overflow_bytes = 0;
        if (e != hipErrorOutOfMemory) return hip_fail(h, e, "build run blocks on the device");
        (void)hipGetLastError();  // no room for the run blocks beside the planes: the planes are gone now, the host builder takes over
        if (std::getenv("MSBWT_VERBOSE")) std::fprintf(stderr, "[msbwt] run blocks: out of memory on the device path -- built on the host\n");
    }
    Totals t;
    if (!compute_totals(rle, n, &t)) return fail(h, MSBWT_ERR_INVALID_SYMBOL, "RLE stream holds a symbol code >= 6");
    if (t.total > kMaxTotal) return fail(h, MSBWT_ERR_TOO_LARGE, "BWT has 2^40 symbols or more");
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

int rebuild_table(msbwt_rle *h, bool allow_sparse) {
    // (run blocks: their sparse table was built at load time from temporary plane and pair blocks -- build_sparse_for_runs -- and does
    // not depend on the direct table rebuilt here; it goes with the index, or by msbwt_rle_set_sparse_table(0))
    if (h->block_format == kBlocksPlanes) release_sparse(h);
    DirectTable &t = h->table;
    t.release();
    // Automatic depths come from ONE decision (table_policy.hpp, pinned by a CPU test through
    // msbwt_auto_table_depths): beside a pair index the flat table is built as deep as the packed one needs.
    const bool automatic = h->wanted_table_depth < 0;
    int depth = h->wanted_table_depth;
    bool pack = h->pair.blocks != nullptr && h->wanted_table_packed > 0;  // an explicit depth is packed only on request
    if (automatic && h->planned) {  // a memory budget is in force: the plan has sized the table (table_policy.hpp, plan_index)
        depth = h->plan.flat;
        pack = h->plan.packed != 0 && h->pair.blocks != nullptr && h->wanted_table_packed != 0;
    } else if (automatic) {
        size_t free_b = 0, total_b = 0;
        const bool know_free = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        // the table budgets against DISJOINT pair blocks: what overlapping ones take on top was checked against the
        // reserve when they were chosen (choose_pair_stride)
        const TableChoice c = choose_table_depths(h->totals.total, h->nblocks * kBlockBytes, know_free ? uint64_t(free_b) + h->pair.overlap_bytes : 0,
                                                  h->pair.blocks != nullptr, h->wanted_table_packed != 0);
        depth = c.flat;
        pack = c.packed != 0 || (h->pair.blocks != nullptr && h->wanted_table_packed > 0);  // mode 1: whenever a pair index exists
    }
    // The sparse table (sparse_table.hpp) is tried whenever a pair index exists; the automatic direct table then stays small.
    // Should no sparse depth fit (a read set whose error k-mers outnumber the genome's many times over), the direct table is built
    // again as if there were no such thing.
    const bool try_sparse = allow_sparse && h->wanted_sparse != 0 && h->pair.blocks != nullptr && h->block_format == kBlocksPlanes && h->totals.total > 0;
    bool capped = false;
    const int uncapped_depth = depth;
    if (try_sparse && automatic && depth > kDirectDepthBesideSparse) {
        depth = kDirectDepthBesideSparse;
        capped = true;
    }
    // (run blocks behind a sparse table -- built at load time, build_sparse_for_runs: the lean format keeps its flat direct table at depth 13,
    // 1 GB instead of 17, for the queries the sparse table does not serve)
    if (h->block_format == kBlocksRuns && h->sparse.lines && automatic && depth > kDirectDepthBesideSparse) depth = kDirectDepthBesideSparse;
    if (depth <= 0 && !try_sparse) return MSBWT_OK;
    if (depth + 2 > 18) pack = false;
    auto build_flat = [&](int d) -> int {
        const size_t bytes = (size_t(1) << (2 * d)) * 16;
        void *tab = nullptr;
        HIP_TRY(h, hipMalloc(&tab, bytes));
        hipError_t e = launch_build_table(view_of(h), d, tab, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipFree(tab);
            if (e == hipErrorNotSupported) return MSBWT_OK;  // kernel set without a table
            return hip_fail(h, e, "build suffix table");
        }
        t.entries = tab;
        t.depth = d;
        t.bytes = bytes;
        return rebuild_filter(h);  // from the flat table, before it may be packed away
    };
    int rc = depth > 0 ? build_flat(depth) : MSBWT_OK;
    if (rc) return rc;
    if (try_sparse) {
        uint64_t allowance = kNoBudget;
        if (h->planned) {  // what the budget leaves once blocks, pair blocks and the direct table are paid for
            const uint64_t direct = (pack && t.entries) ? packed_table_bytes(depth + 2) : uint64_t(t.bytes);
            const uint64_t held = h->nblocks * kBlockBytes + h->pair.bytes + direct;
            allowance = h->memory_budget > held ? h->memory_budget - held : 0;
        }
        rc = build_sparse(h, (pack && t.entries) ? packed_table_bytes(depth + 2) : 0, allowance, t.entries ? depth + (pack ? 2 : 0) : 0, (capped && pack) ? uncapped_depth : 0);
        if (rc) return rc;
        if (!h->sparse.lines && capped) {  // no depth fit: the direct table as if there were no sparse one (the distinct counts stay on record)
            const SparseBuildReport counted = h->sparse_report;
            const int again = rebuild_table(h, false);
            h->sparse_report = counted;
            return again;
        }
    }
    // Beside a sparse table the direct table serves the queries SHORTER than that table's entries (and those with '$' / 'N' among their
    // last symbols).  Capped at packed depth 15 those lose against the index without a sparse table (round 6, human scale, present
    // k-mers: k = 17 2.5 x, k = 19 1.8 x, k = 21 1.5 x slower than behind the packed depth-17 table) -- so where HBM is plentiful (a
    // chr20-sized index: 15 GB of 288) the deep direct table is kept AS WELL: nothing is lost for any k.  Not under a memory budget
    // (the plan has sized the table), and not where it would take the eighth of the device left to the caller's batches (deep_direct_fits);
    // there build_sparse has tried a second, shallower sparse level instead.  Nor where a two-tier table would then be no deeper than the
    // direct table its filter sends queries to (sparse_tier_fits_direct: a declared k = 16 or 17).
    if (capped && h->sparse.lines && !h->sparse2.lines && t.entries && pack && (!h->sparse.tier || sparse_tier_fits_direct(h->sparse.depth, uncapped_depth + 2)) &&
        deep_direct_fits(h, uncapped_depth)) {
        t.release();
        depth = uncapped_depth;
        rc = build_flat(depth);
        if (rc) return rc;
    }
    if (!t.entries || !pack) return rc;
    // Packed form, two levels deeper (kernels.hpp, launch_pack_table): every level removes a line fetch
    // per query, and the first step after a shallow table is the expensive one (wide ranges straddle
    // blocks).  Needs the pair index.
    const uint64_t pbytes = packed_table_bytes(depth + 2);
    void *packed = nullptr;
    unsigned long long *d_cnt = pack_scratch(h);  // [0] escape lines, [1] side cursor
    unsigned long long escapes = 0;
    hipError_t e = hipMalloc(&packed, pbytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, 16, h->stream);
    if (e == hipSuccess) e = launch_pack_table(view_of(h), depth, t.entries, packed, d_cnt, nullptr, nullptr, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&escapes, d_cnt, sizeof escapes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    // Escape lines (some delta beyond 16 bits: the suffixes of high-copy repeats) get their ranges as flat entries in a side
    // array, 512 bytes per line, filled by a second pass over those lines only.  Optional: without it (no memory, or
    // MSBWT_TABLE_SIDE=0) their queries search from scratch.
    void *side = nullptr;
    if (e == hipSuccess && escapes > 0 && h->wanted_table_side != 0) {
        if (hipMalloc(&side, size_t(escapes) * 512) != hipSuccess) {
            (void)hipGetLastError();
            side = nullptr;
        } else {
            e = launch_pack_table(view_of(h), depth, t.entries, packed, nullptr, side, d_cnt + 1, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
    }
    if (e != hipSuccess) {
        if (side) (void)hipFree(side);
        if (packed) (void)hipFree(packed);
        (void)hipGetLastError();
        if (!automatic || h->wanted_table_packed > 0) return hip_fail(h, e, "pack suffix table");
        // optional structure: the handle keeps a flat table -- within the flat table's OWN budget, not the
        // deeper parent that was only meant to be packed away
        const int own = auto_flat_table_depth(h->totals.total, h->nblocks * kBlockBytes);
        if (own < depth) {
            t.release();
            return own > 0 ? build_flat(own) : MSBWT_OK;
        }
        return MSBWT_OK;
    }
    (void)hipFree(t.entries);
    t.entries = packed;
    t.depth = depth + 2;
    t.packed = true;
    t.bytes = pbytes;
    t.side = side;
    t.side_bytes = side ? uint64_t(escapes) * 512 : 0;
    t.lines = pbytes / 128;
    t.escape_lines = escapes;
    if (h->sparse2.lines && h->sparse2.tier && !h->sparse.tier && escapes > 0 && !side) h->sparse2.release();  // (only the second level is two-tier: it alone goes)
    if (h->sparse.lines && (h->sparse.tier || h->sparse2.tier) && escapes > 0 && !side) {
        // the two-tier table sends queries down this table's path, and an escape line without its side entry cannot be followed from
        // there (the query's first symbols are gone): no room for the side array -> the index as if there were no sparse table -- unless
        // that very table was asked for, which is then an error (as an explicit depth that does not fit)
        if (h->wanted_sparse > 0 && h->wanted_tiers == 1 && h->sparse.tier) {
            release_sparse(h);
            return fail(h, MSBWT_ERR_HIP, "the two-tier sparse table of the requested depth cannot be kept: no room for the direct table's side array");
        }
        const SparseBuildReport counted = h->sparse_report;
        const int again = rebuild_table(h, false);
        h->sparse_report = counted;
        return again;
    }
    return MSBWT_OK;
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
    void *scratch = nullptr;
    hipError_t e = hipMalloc(&p.blocks, sz.pair_block_bytes);
    if (e == hipSuccess) e = hipMalloc(&p.super, sz.super_bytes);
    if (e == hipSuccess) e = hipMalloc(&scratch, sz.scratch_bytes);
    if (e == hipSuccess) e = build_pair_index(h->d_blocks, h->nblocks, h->totals.start_index, p.blocks, p.super, scratch, h->stream, stride);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (scratch) (void)hipFree(scratch);
    if (e != hipSuccess) {
        p.release();
        if (h->wanted_pair < 0 && e == hipErrorOutOfMemory) return MSBWT_OK;  // optional structure
        return hip_fail(h, e, "build pair index");
    }
    p.stride = stride;
    p.bytes = sz.pair_block_bytes + sz.super_bytes;
    return MSBWT_OK;
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
    // MSBWT_VERBOSE=1: one stderr line per load stage (the reference logs its load milestones with
    // log::info!, rle_bwt.rs:62,149,347,383)
    const bool verbose = std::getenv("MSBWT_VERBOSE") != nullptr;
    auto clock = std::chrono::steady_clock::now();
    auto stage = [&](const char *what, uint64_t bytes) {
        if (!verbose) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[msbwt] load: %-22s %7.2f s  %8.2f GB in HBM\n", what, std::chrono::duration<double>(now - clock).count(), double(bytes) / 1e9);
        clock = now;
    };
    Totals t{};
    const char *mode = std::getenv("MSBWT_BUILD");
    h->block_format = h->wanted_block_format;
    if (h->block_format == kBlocksRuns) rc = build_run_index(h, rle, n, &t);
    else rc = (mode && std::strcmp(mode, "host") == 0) ? build_on_host(h, rle, n, &t) : build_on_device(h, rle, n, &t);
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
    if (verbose)
        std::fprintf(stderr, "[msbwt] load: %llu symbols, table depth %d, a present %u-mer occurs %.0f times (median), %.2f GB of HBM in all\n",
                     (unsigned long long)t.total, h->table.depth, kProbeSteps, h->typical_width,
                     double(h->nblocks * kBlockBytes + h->overflow_bytes + h->pair.bytes + h->table.bytes + h->sparse.bytes + h->sparse.side_bytes) / 1e9);
    if (verbose)  // where the arrays landed (run-to-run differences of up to 15 % on one box follow the process, not the clocks: profiles/r04_lab)
        std::fprintf(stderr, "[msbwt] load: blocks %p pair blocks %p pair super %p table %p side %p filter %p\n", h->d_blocks, h->pair.blocks,
                     h->pair.super, h->table.entries, h->table.side, static_cast<void *>(h->table.filter));
    h->err.clear();
    return MSBWT_OK;
}

}  // namespace msbwt_capi
