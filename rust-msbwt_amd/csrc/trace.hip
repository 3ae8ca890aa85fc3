// gfx950 (MI355X, CDNA4): the kernels of the traces (trace.hpp) -- what lies between two searches of a batch of walks.  One thread a
// live walk; a workgroup of 256 takes 256 consecutive live walks a trip, every thread of it the same number of trips (the compaction
// has barriers).
//
// Traffic per live walk and round: its 64-byte state in and (a survivor) out, its 4 or 8 counts in, its 4 or 8 next queries out, one
// symbol byte into its own row; a walk that stops writes 26 bytes of outputs.  All of it streams but the row byte and the outputs,
// which scatter by walk number.  Against the 4 or 8 searches of k + 1 symbols a walk that a round costs, this kernel is noise: it is
// written to be read.  One atomic a workgroup and trip (the survivors' places), three a workgroup at its end (the counters).
// One writer per plain store: a walk is in one thread of one round, and its outputs are written by the round that stops it.
// Results do not depend on timing; the order of the survivors does.  No MFMA, no LDS beyond the prefix sum's words.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "trace.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;

__device__ __forceinline__ uint64_t node_mask(uint32_t k) { return (1ull << (2u * k)) - 1ull; }  // k <= 31

// the edge by symbol c out of node w in walk direction `left`, and the node at its other end (the header's table)
__device__ __forceinline__ uint64_t edge_word(uint64_t w, uint32_t c, uint32_t k, bool left) { return left ? (uint64_t(c) << (2u * k)) | w : (w << 2) | uint64_t(c); }
__device__ __forceinline__ uint64_t next_node(uint64_t w, uint32_t c, uint32_t k, bool left) {
    return left ? (uint64_t(c) << (2u * (k - 1u))) | (w >> 2) : ((w << 2) | uint64_t(c)) & node_mask(k);
}

// the four edges of the fan of w at q[0 .. 4) and, in unitig mode, those of its back-fan -- the fan of the other direction -- behind them
__device__ __forceinline__ void write_queries(uint64_t *__restrict__ q, uint64_t w, uint32_t k, bool left, bool back) {
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) q[c] = edge_word(w, c, k, left);
    if (back) {
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) q[4u + c] = edge_word(w, c, k, !left);
    }
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

__global__ __launch_bounds__(kThreads) void k_trace_seed(TraceCall c, uint64_t first_walk, uint64_t walks, TraceWalk *__restrict__ state, uint64_t *__restrict__ queries) {
    const bool left = c.direction == kTraceLeft;
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < walks; j += uint64_t(gridDim.x) * kThreads) {
        const uint64_t walk = first_walk + j, seed = c.seeds[walk - c.first] & node_mask(c.k);
        state[j] = TraceWalk{seed, seed, seed, 0, 0, 0, walk, 0};
        queries[j] = seed;
        write_queries(queries + walks + 4u * j, seed, c.k, left, false);
    }
}

template <bool kRound0>
__global__ __launch_bounds__(kThreads) void k_trace_round(TraceCall c, uint64_t piece_walks, uint64_t live, const TraceWalk *__restrict__ in,
                                                          const uint64_t *__restrict__ counts, TraceWalk *__restrict__ out, uint64_t *__restrict__ queries) {
    __shared__ uint64_t wave_sums[4];
    __shared__ uint64_t block_base;
    const bool left = c.direction == kTraceLeft, unitig = c.mode == kTraceUnitig;
    const uint32_t q = unitig ? 8u : 4u;
    uint64_t sums[2] = {0, 0};  // steps of the walks that stopped here, walks that were no node
    uint64_t longest = 0;
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < live; base += uint64_t(gridDim.x) * kThreads) {  // (the same trips for the whole workgroup)
        const uint64_t j = base + threadIdx.x;
        bool survives = false;
        TraceWalk w{};
        if (j < live) {
            w = in[j];
            const uint64_t *fan_counts = kRound0 ? counts + piece_walks + 4u * j : counts + uint64_t(q) * j;
            uint8_t stop = 0;
            uint32_t stop_fan = uint32_t(w.meta >> 4) & 15u;  // of cur, for a stop that does not enter the candidate
            if (w.walk < c.first || w.walk - c.first >= c.rows || (!kRound0 && w.steps >= c.max_steps)) {
                atomicOr(c.flags, kFlagInternal);  // (a state no round writes: the walk is dropped)
            } else {
                if constexpr (kRound0) {
                    if (counts[j] < c.m) {  // step 0
                        stop = kTraceNotANode;
                        stop_fan = 0;
                        sums[1] += 1;
                    }
                } else {
                    uint32_t back = 0;
                    if (unitig) {
#pragma unroll
                        for (uint32_t s = 0; s < 4u; ++s) back += fan_counts[4u + s] >= c.me ? 1u : 0u;
                    }
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
                    uint32_t fan = 0, width = 0, best = 0;
                    uint64_t best_count = 0;
#pragma unroll
                    for (uint32_t s = 0; s < 4u; ++s) {
                        const uint64_t n = fan_counts[s];
                        if (n >= c.me) {
                            fan |= 1u << s;
                            width += 1;
                            if (n > best_count) {  // (a tie keeps the smaller symbol)
                                best_count = n;
                                best = s;
                            }
                        }
                    }
                    stop_fan = fan;
                    if (!kRound0 && c.targets && w.cur == (c.targets[w.walk - c.first] & node_mask(c.k))) {
                        stop = kTraceTarget;  // step 7
                    } else if (w.steps == c.max_steps) {
                        stop = kTraceMaxSteps;  // step 1
                    } else if (width == 0) {
                        stop = kTraceDeadEnd;  // step 2
                    } else if (width >= 2u && c.mode != kTraceGreedy) {
                        stop = kTraceBranch;  // step 3
                    } else {
                        w.cand = next_node(w.cur, best, c.k, left);
                        w.cand_count = best_count;
                        w.meta = uint64_t(best) | uint64_t(fan) << 4;
                        if (!unitig && w.cand == w.seed) stop = kTraceReturned;  // step 5, nothing to search for
                        else survives = true;
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
                write_queries(queries + uint64_t(q) * p, w.cand, c.k, left, unitig);
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

__global__ __launch_bounds__(kThreads) void k_trace_not_nodes(TraceCall c) {
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < c.rows; i += uint64_t(gridDim.x) * kThreads)
        write_stop(c, i + c.first, kTraceNotANode, 0, 0, c.seeds[i] & node_mask(c.k), 0);
}

}  // namespace

hipError_t launch_trace_seed(const TraceCall &c, uint64_t first_walk, uint64_t walks, TraceWalk *state, uint64_t *queries, hipStream_t stream) {
    if (walks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_trace_seed, dim3(capped_grid(walks, kThreads, kGridCap)), dim3(kThreads), 0, stream, c, first_walk, walks, state, queries);
    return hipGetLastError();
}

hipError_t launch_trace_round(const TraceCall &c, bool round0, uint64_t piece_walks, uint64_t live, const TraceWalk *in, const uint64_t *counts, TraceWalk *out,
                              uint64_t *queries, hipStream_t stream) {
    if (live == 0) return hipSuccess;
    const dim3 grid(capped_grid(live, kThreads, kGridCap)), block(kThreads);
    if (round0)
        hipLaunchKernelGGL(k_trace_round<true>, grid, block, 0, stream, c, piece_walks, live, in, counts, out, queries);
    else
        hipLaunchKernelGGL(k_trace_round<false>, grid, block, 0, stream, c, piece_walks, live, in, counts, out, queries);
    return hipGetLastError();
}

hipError_t launch_trace_not_nodes(const TraceCall &c, hipStream_t stream) {
    if (c.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_trace_not_nodes, dim3(capped_grid(c.rows, kThreads, kGridCap)), dim3(kThreads), 0, stream, c);
    return hipGetLastError();
}

}  // namespace msbwt
