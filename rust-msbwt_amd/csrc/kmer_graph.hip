// gfx950 (MI355X, CDNA4): the edge pass and the degree table of the k-mer graph (kmer_graph.hpp) over the nodes a chunk of the walk staged.
//
// k_graph_edges, per staged node q = {word, l, h}:
//     slot        = rank(l) of the bitmap the counting walk marked (spectrum_rank_below): q's place in ascending k-mer order; word,
//                   count and l go there by plain stores
//     one step    to the four children e = c.q: on plane blocks ONE thread and plane_step (the two lines of l and h, as the walker's
//                   plane step); on run blocks an 8-lane group and constrain_any per symbol (as the walker's run step: correct, not tuned),
//                   after which lane c of the group goes on with child c
//     every child at least min_edge wide is an edge: predecessor bit c at slot, and successor bit (last symbol of q) at
//                   rank(e.l + 1) - 1 -- the last mark at or below e.l is the l of e's prefix p, whose range holds e's
// Four records share a 32-bit word of edge bytes and p's record usually belongs to another chunk, so bits are ORed in by vector
// atomics on that word (zeroed before the walk): a node's predecessor bits in one atomic, each successor bit in one of its own.
// With sink.pred_slot set (the unitig call), every in-edge also stores its predecessor's slot, marks - 1, at the node's own slot, from
// the lane that holds the edge: the word is only ever read for a node with ONE in-edge, which has one writer; where several edges store
// (one thread in turn on plane blocks, lanes of a group on run blocks) whichever value stays is a valid slot below n that nobody reads.
// No address is formed from a range that is not inside [0, total], nor from a slot at or beyond n: kFlagInternal instead.
// Traffic per node: the 24-byte staged record, two plane-block lines (one when l and h share a block), and per rank lookup one
// checkpoint and up to one 128-byte line of the bitmap -- five lookups at most; three 8-byte stores and up to five atomics.
//
// k_graph_degrees folds the finished bytes into the 25 counters: a thread takes a word (four records); per byte the wave agrees on
// the cells it holds -- a ballot per distinct cell, a handful on real data where nearly every node is (1, 1) -- and the first lane of
// each cell adds the ballot's population to the workgroup's LDS table with one LDS atomic; the table is flushed with one global atomic
// per non-zero counter per workgroup.  Integer work: no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "frontier.hpp"
#include "kernels.hpp"
#include "kmer_graph.hpp"
#include "rank_ops.hpp"
#include "slot_bytes.hpp"
#include "spectrum.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;

template <bool kRuns>
__global__ __launch_bounds__(kThreads) void k_graph_edges(const Node *__restrict__ staged, uint64_t m, const uint4 *__restrict__ blocks, const uint4 *__restrict__ overflow,
                                                         uint64_t total, GraphSink sink) {
    constexpr uint32_t kLanes = kRuns ? uint32_t(kGroup) : 1u;  // lanes that work on one node
    constexpr uint32_t kPer = uint32_t(kThreads) / kLanes;
    const uint32_t sub = threadIdx.x % kLanes;
    for (uint64_t base = uint64_t(blockIdx.x) * kPer; base < m; base += uint64_t(gridDim.x) * kPer) {
        const uint64_t i = base + threadIdx.x / kLanes;
        if (i >= m) continue;  // (the same branch in all lanes of a group, here and below)
        const Node nd = staged[i];
        if (!(nd.l < nd.h && nd.h <= total)) {  // (the walk stages nothing else)
            if (sub == 0u) atomicOr(sink.flags, kFlagInternal);
            continue;
        }
        uint64_t nl[4] = {0, 0, 0, 0}, nh[4] = {0, 0, 0, 0};
        if constexpr (kRuns) {
#pragma unroll 1
            for (uint32_t q = 0; q < 4u; ++q) {
                const Range r = constrain_any(1u, blocks, overflow, q == 3u ? 5u : q + 1u, nd.l, nd.h, sub);
                nl[q] = r.l;
                nh[q] = r.h;
            }
        } else {
            plane_step(nd, blocks, nl, nh);
        }
        const uint64_t slot = spectrum_rank_below(sink.bitmap, sink.prefix, nd.l);
        if (slot >= sink.n) {
            if (sub == 0u) atomicOr(sink.flags, kFlagInternal);
            continue;
        }
        if (sub == 0u) {
            if (sink.kmers) sink.kmers[slot] = nd.key;
            if (sink.counts) sink.counts[slot] = nd.h - nd.l;
            if (sink.l) sink.l[slot] = nd.l;
        }
        const uint32_t last = uint32_t(nd.key) & 3u;  // the symbol e's prefix p gains to become e[1..k] = q
        uint32_t pred = 0;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            if (kRuns && c != sub) continue;  // (lane c of a group goes on with child c; lanes 4..7 have none)
            const uint64_t a = nl[c], b = nh[c];
            if (!(a < b && b <= total) || b - a < sink.min_edge) continue;
            const uint64_t marks = spectrum_rank_below(sink.bitmap, sink.prefix, a + 1u);  // p.l <= a: at least one
            if (marks == 0u || marks > sink.n) {
                atomicOr(sink.flags, kFlagInternal);
                continue;
            }
            pred |= 1u << c;
            if (sink.pred_slot) sink.pred_slot[slot] = marks - 1u;
            or_slot_bits(sink.edge_words, marks - 1u, 16u << last);
        }
        if (pred) or_slot_bits(sink.edge_words, slot, pred);
    }
}

// table[5 in + out] += 1 for every record of the n edge bytes
__global__ __launch_bounds__(kThreads) void k_graph_degrees(const uint32_t *__restrict__ edge_words, uint64_t n, unsigned long long *__restrict__ table) {
    __shared__ uint32_t lds_table[32];
    if (threadIdx.x < 32u) lds_table[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwords = (n + 3u) / 4u;  // graph_edge_words(n)
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < nwords; base += uint64_t(gridDim.x) * kThreads) {  // (the same trips for the whole workgroup)
        const uint64_t w = base + threadIdx.x;
        const uint32_t word = w < nwords ? edge_words[w] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t byte = (word >> (8u * j)) & 0xFFu;
            const bool real = w < nwords && w * 4u + j < n;
            const uint32_t cell = uint32_t(__popc(byte & 15u)) * kGraphDegrees + uint32_t(__popc(byte >> 4));
            unsigned long long todo = __ballot(real);
            while (todo != 0ull) {  // (wave-uniform: one trip per distinct cell among the wave's 64 records)
                const int first = __ffsll(todo) - 1;
                const uint32_t its = uint32_t(__shfl(int(cell), first));
                const unsigned long long same = __ballot(real && cell == its);
                if (int(lane) == first) atomicAdd(&lds_table[its], uint32_t(__popcll(same)));
                todo &= ~same;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kGraphTableWords && lds_table[threadIdx.x]) atomicAdd(table + threadIdx.x, (unsigned long long)lds_table[threadIdx.x]);
}

}  // namespace

hipError_t launch_graph_edges(const IndexView &ix, const void *d_staged, uint64_t m, const GraphSink &sink, hipStream_t stream) {
    if (!d_staged || !ix.blocks || !sink.bitmap || !sink.prefix || !sink.edge_words || !sink.flags || sink.min_edge < 1) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    const Node *staged = static_cast<const Node *>(d_staged);
    const uint4 *blocks = static_cast<const uint4 *>(ix.blocks), *overflow = static_cast<const uint4 *>(ix.overflow);
    if (ix.block_format == kBlocksRuns)
        hipLaunchKernelGGL(k_graph_edges<true>, dim3(capped_grid(m, uint64_t(kThreads / kGroup), kGridCap)), dim3(kThreads), 0, stream, staged, m, blocks, overflow, ix.total, sink);
    else
        hipLaunchKernelGGL(k_graph_edges<false>, dim3(capped_grid(m, uint64_t(kThreads), kGridCap)), dim3(kThreads), 0, stream, staged, m, blocks, overflow, ix.total, sink);
    return hipGetLastError();
}

hipError_t launch_graph_degrees(const uint32_t *d_edge_words, uint64_t n, uint64_t *d_table, hipStream_t stream) {
    if (!d_edge_words || !d_table) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_graph_degrees, dim3(capped_grid(graph_edge_words(n), uint64_t(kThreads), kGridCap)), dim3(kThreads), 0, stream, d_edge_words, n,
                       reinterpret_cast<unsigned long long *>(d_table));
    return hipGetLastError();
}

}  // namespace msbwt
