// gfx950 (MI355X, CDNA4): the kernels of the canonical traces (canonical_trace.hpp) -- what lies between two searches of a batch of
// walks through the strand-merged graph.  The frame is trace.hip's: one thread a live walk; a workgroup of 256 takes 256 consecutive
// live walks a trip, every thread of it the same number of trips (the compaction has barriers).
//
// Traffic per live walk and round: its 64-byte state in and (a survivor) out, its 8 + 1 or 16 + 2 counts in, as many next queries
// out, one symbol byte into its own row; a walk that stops writes 26 bytes of outputs.  Twice the counts and queries of trace.hip
// and a handful of bit reversals a walk, against 8 or 16 searches of k + 1 symbols: noise again, and written to be read.  One atomic a
// workgroup and trip (the survivors' places), three a workgroup at its end (the counters).  One writer per plain store.  Results do
// not depend on timing; the order of the survivors does.  No MFMA, no LDS beyond the prefix sum's words.
#include <hip/hip_runtime.h>

#include "canonical.hpp"
#include "canonical_trace.hpp"
#include "kernels.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;

__device__ __forceinline__ uint64_t node_mask(uint32_t k) { return (1ull << (2u * k)) - 1ull; }  // k <= 31

// the header's table: the edge by symbol c out of node w in walk direction `left`, and the node at its other end
__device__ __forceinline__ uint64_t edge_word(uint64_t w, uint32_t c, uint32_t k, bool left) { return left ? (uint64_t(c) << (2u * k)) | w : (w << 2) | uint64_t(c); }
__device__ __forceinline__ uint64_t next_node(uint64_t w, uint32_t c, uint32_t k, bool left) {
    return left ? (uint64_t(c) << (2u * (k - 1u))) | (w >> 2) : ((w << 2) | uint64_t(c)) & node_mask(k);
}
__device__ __forceinline__ bool palindrome(uint64_t w, uint32_t len) { return w == reverse_complement_2bit(w, len); }

// The symbol by which the fan of w can reach a palindrome: the far end begins (RIGHT) with w's second symbol and ends with c, or ends
// (LEFT) with w's last but one and begins with c.  k = 1 has no such symbol, and no node clause: any c serves.
__device__ __forceinline__ uint32_t mirror_symbol(uint64_t w, uint32_t k, bool left) {
    if (k < 2u) return 0u;
    return 3u - uint32_t((left ? w >> 2 : w >> (2u * (k - 2u))) & 3u);
}

// the fan of w: its four edges and their reverse complements at q[0 .. 8), and the one far end the node clause asks about at *far
__device__ __forceinline__ void write_fan(uint64_t *__restrict__ q, uint64_t *__restrict__ far, uint64_t w, uint32_t k, bool left) {
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        const uint64_t e = edge_word(w, c, k, left);
        q[c] = e;
        q[4u + c] = reverse_complement_2bit(e, k + 1u);
    }
    *far = next_node(w, mirror_symbol(w, k, left), k, left);
}

// The fan of w in D from the counts of write_fan's queries: the edge by c is there when cc(e) >= me and its far end is a node, which
// only a palindromic far end (far_count: its count, read with the node clause only) can fail to be.
struct Fan {
    uint32_t bits = 0, width = 0, best = 0;
    uint64_t best_count = 0;  // the largest cc, of the smallest symbol that has it
};
__device__ __forceinline__ Fan read_fan(const TraceCall &c, bool node_clause, uint64_t w, bool left, const uint64_t *__restrict__ counts, uint64_t far_count) {
    Fan f;
    const uint32_t mirror = mirror_symbol(w, c.k, left);
#pragma unroll
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint64_t n = palindrome(edge_word(w, s, c.k, left), c.k + 1u) ? counts[s] : counts[s] + counts[4u + s];
        bool edge = n >= c.me;
        if (node_clause && s == mirror && far_count < c.m && palindrome(next_node(w, s, c.k, left), c.k)) edge = false;
        if (edge) {
            f.bits |= 1u << s;
            f.width += 1;
            if (n > f.best_count) {  // (a tie keeps the smaller symbol)
                f.best_count = n;
                f.best = s;
            }
        }
    }
    return f;
}

// a walk's five outputs behind its row of symbols
__device__ __forceinline__ void write_stop(const TraceCall &c, uint64_t walk, uint8_t stop, uint64_t steps, uint64_t edge_sum, uint64_t last, uint32_t fan) {
    const uint64_t i = walk - c.first;
    if (c.steps) c.steps[i] = steps;
    if (c.stops) c.stops[i] = stop;
    if (c.edge_sums) c.edge_sums[i] = edge_sum;
    if (c.last) c.last[i] = last;
    if (c.fans) c.fans[i] = uint8_t(fan);
}

__global__ __launch_bounds__(kThreads) void k_canonical_trace_seed(TraceCall c, uint64_t first_walk, uint64_t walks, TraceWalk *__restrict__ state,
                                                                   uint64_t *__restrict__ queries) {
    const bool left = c.direction == kTraceLeft;
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < walks; j += uint64_t(gridDim.x) * kThreads) {
        const uint64_t walk = first_walk + j, seed = c.seeds[walk - c.first] & node_mask(c.k);
        state[j] = TraceWalk{seed, seed, seed, 0, 0, 0, walk, 0};
        queries[2u * j] = seed;
        queries[2u * j + 1u] = reverse_complement_2bit(seed, c.k);
        write_fan(queries + 2u * walks + 8u * j, queries + 10u * walks + j, seed, c.k, left);
    }
}

template <bool kRound0>
__global__ __launch_bounds__(kThreads) void k_canonical_trace_round(TraceCall c, bool node_clause, uint64_t piece_walks, uint64_t live, const TraceWalk *__restrict__ in,
                                                                    const uint64_t *__restrict__ counts, TraceWalk *__restrict__ out, uint64_t *__restrict__ queries) {
    __shared__ uint64_t wave_sums[4];
    __shared__ uint64_t block_base;
    const bool left = c.direction == kTraceLeft, unitig = c.mode == kTraceUnitig;
    const uint32_t f = unitig ? 16u : 8u, e = unitig ? 2u : 1u;
    uint64_t sums[2] = {0, 0};  // steps of the walks that stopped here, walks that were no node
    uint64_t longest = 0;
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < live; base += uint64_t(gridDim.x) * kThreads) {  // (the same trips for the whole workgroup)
        const uint64_t j = base + threadIdx.x;
        bool survives = false;
        TraceWalk w{};
        if (j < live) {
            w = in[j];
            const uint64_t *fan_counts = kRound0 ? counts + 2u * piece_walks + 8u * j : counts + uint64_t(f) * j;
            const uint64_t *far_counts = kRound0 ? counts + 10u * piece_walks + j : counts + uint64_t(f) * piece_walks + uint64_t(e) * j;
            uint8_t stop = 0;
            uint32_t stop_fan = uint32_t(w.meta >> 4) & 15u;  // of cur, for a stop that does not enter the candidate
            if (w.walk < c.first || w.walk - c.first >= c.rows || (!kRound0 && w.steps >= c.max_steps)) {
                atomicOr(c.flags, kFlagInternal);  // (a state no round writes: the walk is dropped)
            } else {
                if constexpr (kRound0) {
                    const uint64_t cc = palindrome(w.seed, c.k) ? counts[2u * j] : counts[2u * j] + counts[2u * j + 1u];
                    if (cc < c.m) {  // step 0
                        stop = kTraceNotANode;
                        stop_fan = 0;
                        sums[1] += 1;
                    }
                } else {
                    const uint32_t back = unitig ? read_fan(c, node_clause, w.cand, !left, fan_counts + 8u, node_clause ? far_counts[1] : 0).width : 0u;
                    if (back >= 2u) {
                        stop = kTraceMerge;  // step 4
                    } else if (w.cand == w.seed) {
                        stop = kTraceReturned;  // step 5 (unitig mode; the other modes saw it when they chose)
                    } else {  // step 6
                        const uint32_t sym = uint32_t(w.meta) & 3u;
                        if (c.symbols) c.symbols[(w.walk - c.first) * c.max_steps + w.steps] = uint8_t(sym + 1u + (sym == 3u ? 1u : 0u));
                        w.edge_sum += w.cand_count;
                        w.steps += 1;
                        w.cur = w.cand;
                    }
                }
                if (!stop) {
                    // the fan of the node just entered (round 0: of the seed)
                    const Fan fan = read_fan(c, node_clause, w.cur, left, fan_counts, node_clause ? far_counts[0] : 0);
                    stop_fan = fan.bits;
                    if (!kRound0 && c.targets && w.cur == (c.targets[w.walk - c.first] & node_mask(c.k))) {
                        stop = kTraceTarget;  // step 7
                    } else if (w.steps == c.max_steps) {
                        stop = kTraceMaxSteps;  // step 1
                    } else if (fan.width == 0) {
                        stop = kTraceDeadEnd;  // step 2
                    } else if (fan.width >= 2u && c.mode != kTraceGreedy) {
                        stop = kTraceBranch;  // step 3
                    } else {
                        w.cand = next_node(w.cur, fan.best, c.k, left);
                        w.cand_count = fan.best_count;
                        w.meta = uint64_t(fan.best) | uint64_t(fan.bits) << 4;
                        if (unitig && (palindrome(w.cur, c.k) || palindrome(w.cand, c.k) || palindrome(edge_word(w.cur, fan.best, c.k, left), c.k + 1u)))
                            stop = kCanonicalTraceMirror;  // step 3b: the link is one of the two cuts, nothing to search for
                        else if (!unitig && w.cand == w.seed)
                            stop = kTraceReturned;  // step 5, nothing to search for
                        else
                            survives = true;
                    }
                }
                if (stop) {
                    write_stop(c, w.walk, stop, w.steps, w.edge_sum, w.cur, stop_fan);
                    sums[0] += w.steps;
                    longest = w.steps > longest ? w.steps : longest;
                }
            }
        }
        uint64_t all = 0;
        const uint64_t before = block_exclusive_sum(uint64_t(survives ? 1 : 0), wave_sums, &all);
        if (threadIdx.x == 0) block_base = all ? atomicAdd(c.counters + kTraceLive, (unsigned long long)all) : 0;
        __syncthreads();
        const uint64_t p = block_base + before;
        if (survives) {
            if (p < live) {
                out[p] = w;
                uint64_t *far = queries + uint64_t(f) * piece_walks + uint64_t(e) * p;
                write_fan(queries + uint64_t(f) * p, far, w.cand, c.k, left);
                if (unitig) write_fan(queries + uint64_t(f) * p + 8u, far + 1, w.cand, c.k, !left);
            } else {
                atomicOr(c.flags, kFlagInternal);  // (more survivors than walks)
            }
        }
        __syncthreads();  // block_base is free again
    }
    static_assert(kTraceNotNodes == kTraceSteps + 1, "the two sums lie side by side");
    add_to_counters(c.counters, kTraceSteps, sums);
    longest = wave_max(longest);
    if ((threadIdx.x & 63u) == 0u && longest) atomicMax(c.counters + kTraceLongest, (unsigned long long)longest);
}

}  // namespace

hipError_t launch_canonical_trace_seed(const TraceCall &c, uint64_t first_walk, uint64_t walks, TraceWalk *state, uint64_t *queries, hipStream_t stream) {
    if (walks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_canonical_trace_seed, dim3(capped_grid(walks, kThreads, kGridCap)), dim3(kThreads), 0, stream, c, first_walk, walks, state, queries);
    return hipGetLastError();
}

hipError_t launch_canonical_trace_round(const TraceCall &c, bool round0, bool node_clause, uint64_t piece_walks, uint64_t live, const TraceWalk *in,
                                        const uint64_t *counts, TraceWalk *out, uint64_t *queries, hipStream_t stream) {
    if (live == 0) return hipSuccess;
    if (live > piece_walks) return hipErrorInvalidValue;  // (the blocks hold piece_walks walks)
    const dim3 grid(capped_grid(live, kThreads, kGridCap)), block(kThreads);
    if (round0)
        hipLaunchKernelGGL(k_canonical_trace_round<true>, grid, block, 0, stream, c, node_clause, piece_walks, live, in, counts, out, queries);
    else
        hipLaunchKernelGGL(k_canonical_trace_round<false>, grid, block, 0, stream, c, node_clause, piece_walks, live, in, counts, out, queries);
    return hipGetLastError();
}

}  // namespace msbwt
