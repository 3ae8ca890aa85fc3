// gfx950 builder of the sparse suffix table (sparse_table.hpp): the frontier walk (frontier_walk.hpp) with the index's own rank code,
// from the non-empty entries of the flat direct table (depth p; none: from the root) to the table's depth.
//
// A pair step takes every node two symbols further -- all 16 children of a node come from the same one or two pair-block lines (a
// line holds the counts of all 16 pairs), so a level costs about one random line per node, not 32 ranks -- and the odd last level is
// a plane step.  The order in which children reach a frontier means nothing: the table is hashed.  Both passes are walks of their
// own, chunked, retried and descended by the walker as the data and the scratch demand; this file has their two sinks:
//     sizing  takes nothing, and tallies at EVERY level how many children are 255 or more wide and how many exactly 1 wide: with the
//             nodes per depth, that is the report the depth is chosen from
//     fill    puts each child of the last level into its bucket (an atomic slot counter per bucket; a full bucket sends the entry
//             on to the next one).  A chunk that overflows a frontier has not reached the last level, so the table has seen nothing
//             of it when the walker takes it again.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "frontier_walk.hpp"
#include "sparse_build.hpp"

namespace msbwt {
namespace {

static_assert(kSparseMaxDepth < int(kWalkMaxDepth), "the walk reaches every depth a table can have");
// the fill sink's words of the cursor block (kept from chunk to chunk)
constexpr int kSideCursor = kWalkSink, kDisplaced = kWalkSink + 1, kFailed = kWalkSink + 2, kFiltered = kWalkSink + 3;

struct CountSink : PlainSink {  // the sizing pass
    struct Seen {
        uint32_t wide = 0, single = 0;  // a bit per child
    };
    __device__ __forceinline__ void see(Seen &s, uint64_t width, uint32_t p) const {
        s.wide |= (width >= kSparseEscapeWidth ? 1u : 0u) << p;
        s.single |= (width == 1u ? 1u : 0u) << p;
    }
    __device__ __forceinline__ void tally(const Seen &s, unsigned long long *at_depth) const {
        block_add(uint32_t(__popc(s.wide)), at_depth);
        block_add(uint32_t(__popc(s.single)), at_depth + kWalkTallyStride);
    }
};

struct FillEnv : PlainSink {  // the fill pass
    uint4 *lines;        // the table (zeroed)
    uint32_t *counts;    // slot counter per bucket
    uint4 *side;
    uint32_t nbuckets, probe, n;  // n = 2 depth
    uint64_t nside;      // entries the side array holds
    uint32_t tier;       // two-tier form: ranges 1 wide set filter bits in their own bucket instead of taking an entry
    __device__ __forceinline__ void take(Thread &, uint32_t *, unsigned long long *cur, uint64_t key, uint64_t nl, uint64_t nh, uint64_t &) const;
};

// stores one entry into slot `slot` of a bucket line: tag word, l, then the width and the tag's high byte wherever the layout keeps them
__device__ __forceinline__ void sparse_store(uint32_t *line, const SparseLayout &L, uint32_t slot, uint32_t tag, uint32_t tag_hi, uint64_t lval, uint32_t width) {
    uint8_t *bytes = reinterpret_cast<uint8_t *>(line);
    line[slot] = L.width_byte ? tag : tag | (width << kSparseWidthShift);
    line[L.l_lo_word + slot] = uint32_t(lval);
    bytes[L.l_hi_byte + slot] = uint8_t(lval >> 32);
    if (L.width_byte) bytes[L.width_byte + slot] = uint8_t(width);
    if (L.tag_hi_byte) bytes[L.tag_hi_byte + slot] = uint8_t(tag_hi);
}

// puts the entry of (key, [nl, nh)) into its bucket; `cur`: the cursor block (side cursor, displaced, failed)
__device__ __forceinline__ void sparse_insert(const FillEnv &env, uint64_t key, uint64_t nl, uint64_t nh, unsigned long long *cur) {
    const uint64_t x = sparse_mix(key, env.n);
    uint32_t b = sparse_bucket(x, env.n, env.nbuckets);
    const bool tier = env.tier != 0u;
    const SparseLayout L = sparse_layout(env.n >> 1, tier);  // launch-uniform: the layout follows the depth and the form (sparse_table.hpp)
    const uint32_t tag = sparse_tag(x, L), tag_hi = sparse_tag_hi(x, L);
    if (tier && nh - nl == 1u) {  // occurs once: four bits of one filter word of its OWN bucket (never displaced), no entry
        const uint32_t f = sparse_filter_hash(tag);
        atomicOr(reinterpret_cast<uint32_t *>(env.lines + uint64_t(b) * 8u) + L.filter_word + sparse_filter_word(f), sparse_filter_mask(f));
        atomicAdd(cur + kFiltered, 1ull);
        return;
    }
    uint64_t lval = nl;
    uint32_t wf = uint32_t(nh - nl);
    if (nh - nl >= kSparseEscapeWidth) {
        const uint64_t idx = atomicAdd(cur + kSideCursor, 1ull);
        if (idx >= env.nside) {  // (more wide ranges than the sizing pass counted: never on a consistent build -- refuse rather than write outside)
            atomicOr(cur + kFailed, 2ull);
            return;
        }
        env.side[idx] = make_uint4(uint32_t(nl), uint32_t(nl >> 32), uint32_t(nh), uint32_t(nh >> 32));
        lval = idx;
        wf = kSparseEscapeWidth;
    }
    for (uint32_t dist = 0; dist <= env.probe; ++dist, ++b) {
        const uint32_t slot = atomicAdd(env.counts + b, 1u);
        if (slot < L.slots) {
            sparse_store(reinterpret_cast<uint32_t *>(env.lines + uint64_t(b) * 8u), L, slot, tag, tag_hi, lval, wf);
            if (dist != 0u) atomicAdd(cur + kDisplaced, 1ull);
            return;
        }
    }
    atomicOr(cur + kFailed, 1ull);
}

__device__ __forceinline__ void FillEnv::take(Thread &, uint32_t *, unsigned long long *cur, uint64_t key, uint64_t nl, uint64_t nh, uint64_t &) const {
    sparse_insert(*this, key, nl, nh, cur);
}

// the header of every bucket: how many entries wanted it
__global__ __launch_bounds__(256) void k_sparse_headers(uint4 *__restrict__ lines, const uint32_t *__restrict__ counts, uint64_t nlines, uint32_t header_byte) {
    for (uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; b < nlines; b += uint64_t(gridDim.x) * blockDim.x)
        reinterpret_cast<uint16_t *>(lines + b * 8u)[header_byte / 2] = uint16_t(min(counts[b], 0xFFFFu));
}

void keep_walk(const WalkRecord &rec, uint64_t (&out)[3]) {  // chunks, retries, descents: as the report has them
    out[0] = rec.chunks;
    out[1] = rec.retries;
    out[2] = rec.descents;
}

}  // namespace

size_t sparse_work_bytes(uint64_t total, uint64_t free_bytes, uint64_t wanted_nodes) {
    return size_t(walk_work_bytes(walk_frontier_nodes(total, free_bytes, wanted_nodes)));
}

hipError_t sparse_count_levels(const IndexView &ix, const void *flat_entries, int flat_depth, int max_depth, void *d_work, size_t work_bytes,
                               SparseBuildReport *report, hipStream_t stream) {
    if (!ix.pair_blocks || !ix.pair_super || ix.block_format != kBlocksPlanes || max_depth > kSparseMaxDepth || flat_depth < 0 || flat_depth >= max_depth)
        return hipErrorInvalidValue;
    if (flat_entries == nullptr) flat_depth = 0;
    Walker<CountSink, false> walker(ix, flat_entries, flat_depth, uint32_t(max_depth), 1, CountSink{}, d_work, walk_nodes_in(work_bytes), stream);
    const hipError_t e = walker.run();
    if (e != hipSuccess) return e;
    const WalkRecord &rec = walker.record();
    *report = SparseBuildReport{};
    report->parent_depth = int(walker.seed_depth());
    for (int d = 0; d <= kSparseMaxDepth; ++d) {
        report->distinct[d] = rec.nodes[d];
        report->escapes[d] = rec.tally[0][d];
        report->singles[d] = rec.tally[1][d];
    }
    keep_walk(rec, report->sizing_walk);
    return hipSuccess;
}

hipError_t sparse_fill(const IndexView &ix, const void *flat_entries, int flat_depth, int depth, bool tier, void *lines, uint64_t nbuckets, uint32_t probe, void *side,
                       uint64_t nside, void *d_counts, void *d_work, size_t work_bytes, SparseBuildReport *report, hipStream_t stream) {
    if (flat_entries == nullptr) flat_depth = 0;
    if (!ix.pair_blocks || !lines || !d_counts || depth < kSparseMinDepth || depth > kSparseMaxDepth || flat_depth >= depth || nbuckets == 0 ||
        nbuckets + probe > 0xFFFFFFFFull || int(probe) > sparse_probe_limit(depth, nbuckets) || (tier && depth > kTierMaxDepth))
        return hipErrorInvalidValue;
    const uint64_t nlines = nbuckets + probe;
    hipError_t e = hipMemsetAsync(lines, 0, nlines * 128, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, nlines * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const FillEnv env{{}, static_cast<uint4 *>(lines), static_cast<uint32_t *>(d_counts), static_cast<uint4 *>(side), uint32_t(nbuckets), probe, uint32_t(2 * depth),
                      side ? nside : 0, tier ? 1u : 0u};
    Walker<FillEnv, false> walker(ix, flat_entries, flat_depth, uint32_t(depth), 1, env, d_work, walk_nodes_in(work_bytes), stream);
    if ((e = walker.run()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sparse_headers, dim3(uint32_t(std::min<uint64_t>((nlines + 255) / 256, 2048))), dim3(256), 0, stream, static_cast<uint4 *>(lines),
                       static_cast<const uint32_t *>(d_counts), nlines, sparse_layout(uint32_t(depth), tier).header_byte);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    keep_walk(walker.record(), report->fill_walk);
    if (walker.cursor(kFailed) != 0) return hipErrorInvalidValue;  // some entry found no slot (or more wide ranges than counted): more buckets, please
    report->depth = depth;
    report->nbuckets = nbuckets;
    report->nescapes = walker.cursor(kSideCursor);
    report->displaced = walker.cursor(kDisplaced);
    report->tier = tier;
    report->filtered = walker.cursor(kFiltered);
    report->entries = report->distinct[depth] - (tier ? report->filtered : 0ull);
    return hipSuccess;
}

}  // namespace msbwt
