// gfx950 (MI355X, CDNA4): the kernels of the bridges (bridges.hpp) -- what lies between two searches of a frontier of walks.  One
// thread a state (decide, weigh, scatter) or a pair (seed, start, verdict), workgroups of 256 striding over what the grid cap leaves.
//
// Traffic per state and round: its head and its 4 counts in (decide), a word of masks out; a scan word out, scanned, and in again; then
// per child the parent's row in and out -- 8 + ceil(max_steps / 32) words -- and 4 queries out, per bridge a row of the outputs.  Against
// the 4 searches of k + 1 symbols a state that a round costs this is noise; it is written to be read.  The decide kernel's additions
// to a pair's two counters are one 64-bit atomic a wave where the wave holds states of one pair (the rule once a frontier is wide), the
// sums are order-free.  Every store is a vector store with one writer.  No barrier outside the counters' sums, no LDS beyond theirs,
// no MFMA.  Results depend on no timing: a child's slot is the exclusive scan of the weights before it.
#include <hip/hip_runtime.h>

#include "bridges.hpp"
#include "kernels.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;  // the trace kernels'
constexpr uint64_t kNoPair = ~0ull;

__device__ __forceinline__ uint64_t node_mask(uint32_t k) { return (1ull << (2u * k)) - 1ull; }  // k <= 31

// the edge by symbol c out of node w in walk direction `left`, and the node at its other end (the header's table, "traces")
__device__ __forceinline__ uint64_t edge_word(uint64_t w, uint32_t c, uint32_t k, bool left) { return left ? (uint64_t(c) << (2u * k)) | w : (w << 2) | uint64_t(c); }
__device__ __forceinline__ uint64_t next_node(uint64_t w, uint32_t c, uint32_t k, bool left) {
    return left ? (uint64_t(c) << (2u * (k - 1u))) | (w >> 2) : ((w << 2) | uint64_t(c)) & node_mask(k);
}
__device__ __forceinline__ void write_queries(uint64_t *__restrict__ q, uint64_t w, uint32_t k, bool left) {
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) q[c] = edge_word(w, c, k, left);
}
__device__ __forceinline__ uint8_t code_of(uint32_t sym) { return uint8_t(sym + 1u + (sym == 3u ? 1u : 0u)); }  // 1 2 3 5

// the place of a state's pair in the piece's table, or kNoPair for a pair the piece or the call's arrays do not hold
__device__ __forceinline__ uint64_t pair_slot(const BridgeCall &c, const BridgePiece &p, uint64_t pair) {
    return pair < p.first_pair || pair - p.first_pair >= p.pairs || pair < c.first || pair - c.first >= c.rows ? kNoPair : pair - p.first_pair;
}

// a state's scan word once its masks stand and its pair has its verdict: children of a pair that goes on | bridges << 32
__device__ __forceinline__ uint64_t weight_of(const BridgeCall &c, const BridgePiece &p, const uint64_t *__restrict__ s) {
    const uint64_t q = pair_slot(c, p, s[kBridgePair]), masks = s[kBridgeMasks];
    if (q == kNoPair) return 0;
    const uint64_t children = p.table[q * kBridgePairWords + kPairAlive] ? uint64_t(__popc(uint32_t(masks) & 15u)) : 0ull;
    return children | uint64_t(__popc(uint32_t(masks >> 4) & 15u)) << 32;
}

__global__ __launch_bounds__(kThreads) void k_bridge_seed(BridgeCall c, BridgePiece p, uint64_t *__restrict__ state, uint64_t *__restrict__ queries) {
    const bool left = c.direction == kBridgeLeft;
    const uint64_t stride = uint64_t(gridDim.x) * kThreads, at = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    for (uint64_t j = at; j < p.pairs; j += stride) {
        const uint64_t pair = p.first_pair + j, seed = c.seeds[pair - c.first] & node_mask(c.k);
        uint64_t *s = state + j * p.words;
        for (uint64_t w = 0; w < p.words; ++w) s[w] = 0;
        s[kBridgePair] = pair;
        s[kBridgeNode] = seed;
        queries[j] = seed;
        queries[p.pairs + j] = c.targets[pair - c.first] & node_mask(c.k);
        write_queries(queries + 2u * p.pairs + 4u * j, seed, c.k, left);
    }
    const uint64_t base = (p.first_pair - c.first) * c.max_paths;  // unused rows say 0
    for (uint64_t e = at; e < p.pairs * c.max_paths; e += stride) {
        if (c.lengths) c.lengths[base + e] = 0;
        if (c.edge_sums) c.edge_sums[base + e] = 0;
    }
}

// a pair's four outputs behind its rows
__device__ __forceinline__ void write_stop(const BridgeCall &c, uint64_t pair, uint8_t stop, uint64_t found, uint64_t depth, uint64_t live) {
    const uint64_t i = pair - c.first;
    if (c.found) c.found[i] = found;
    if (c.stops) c.stops[i] = stop;
    if (c.depths) c.depths[i] = depth;
    if (c.live) c.live[i] = live;
}

__global__ __launch_bounds__(kThreads) void k_bridge_start(BridgeCall c, BridgePiece p, const uint64_t *__restrict__ counts) {
    uint64_t alive[1] = {0};
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < p.pairs; j += uint64_t(gridDim.x) * kThreads) {
        const uint8_t stop = counts[j] < c.m ? kBridgeNoSeed : counts[p.pairs + j] < c.m ? kBridgeNoTarget : c.max_steps == 0 ? kBridgeMaxSteps : 0;  // step 0
        unsigned long long *t = p.table + j * kBridgePairWords;
        t[kPairChildren] = t[kPairBridges] = t[kPairFound] = t[kPairBase] = 0;
        t[kPairFirst] = j;
        t[kPairAlive] = stop ? 0 : 1;
        if (stop) write_stop(c, p.first_pair + j, stop, 0, 0, stop == kBridgeMaxSteps ? 1 : 0);
        else alive[0] += 1;
    }
    add_to_counters(c.counters, kBridgeAlive, alive);
}

__global__ __launch_bounds__(kThreads) void k_bridge_decide(BridgeCall c, BridgePiece p, uint64_t round, uint64_t live, uint64_t *__restrict__ state,
                                                            const uint64_t *__restrict__ fan_counts) {
    const bool left = c.direction == kBridgeLeft;
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < live; base += uint64_t(gridDim.x) * kThreads) {  // (the same trips for the whole wave)
        const uint64_t j = base + threadIdx.x;
        uint64_t q = kNoPair;
        uint32_t children = 0, bridges = 0;
        if (j < live) {
            uint64_t *s = state + j * p.words;
            const uint64_t pair = s[kBridgePair];
            q = pair_slot(c, p, pair);
            if (q == kNoPair || s[kBridgeSteps] + 1 != round || round > c.max_steps) {
                atomicOr(c.flags, kFlagInternal);  // (a state no round writes: it is dropped)
                s[kBridgeMasks] = 0;
                q = kNoPair;
            } else {
                uint32_t child_mask = 0, bridge_mask = 0;
                if (p.table[q * kBridgePairWords + kPairAlive]) {
                    const uint64_t node = s[kBridgeNode], target = c.targets[pair - c.first] & node_mask(c.k);
#pragma unroll
                    for (uint32_t sym = 0; sym < 4u; ++sym) {
                        if (fan_counts[4u * j + sym] < c.me) continue;
                        if (round >= c.lo && next_node(node, sym, c.k, left) == target) bridge_mask |= 1u << sym;
                        else child_mask |= 1u << sym;
                    }
                }
                s[kBridgeMasks] = child_mask | bridge_mask << 4;
                children = __popc(child_mask);
                bridges = __popc(bridge_mask);
                if (j == 0 || state[(j - 1) * p.words + kBridgePair] != pair) p.table[q * kBridgePairWords + kPairFirst] = j;
            }
        }
        // the pair's two counters: the wave's sums at once where its states with anything to add are of one pair
        const bool adds = (children | bridges) != 0u;
        const unsigned long long who = __ballot(adds);
        if (who == 0ull) continue;  // (uniform over the wave)
        const int lead = __ffsll(who) - 1;
        const uint64_t lead_q = __shfl(q, lead);
        if (__all(!adds || q == lead_q)) {
            const uint32_t all_children = wave_sum(children), all_bridges = wave_sum(bridges);
            if (int(threadIdx.x & 63u) == lead) {
                if (all_children) atomicAdd(p.table + q * kBridgePairWords + kPairChildren, (unsigned long long)all_children);
                if (all_bridges) atomicAdd(p.table + q * kBridgePairWords + kPairBridges, (unsigned long long)all_bridges);
            }
        } else if (adds) {
            if (children) atomicAdd(p.table + q * kBridgePairWords + kPairChildren, (unsigned long long)children);
            if (bridges) atomicAdd(p.table + q * kBridgePairWords + kPairBridges, (unsigned long long)bridges);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_bridge_verdict(BridgeCall c, BridgePiece p, uint64_t round) {
    uint64_t sums[2] = {0, 0};  // walk-steps expanded, bridges found
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < p.pairs; j += uint64_t(gridDim.x) * kThreads) {
        unsigned long long *t = p.table + j * kBridgePairWords;
        if (!t[kPairAlive]) continue;
        const uint64_t children = t[kPairChildren], bridges = t[kPairBridges], found = t[kPairFound] + bridges;
        t[kPairBase] = t[kPairFound];
        t[kPairFound] = found;
        t[kPairChildren] = t[kPairBridges] = 0;
        sums[0] += children + bridges;
        sums[1] += bridges;
        const uint8_t stop = found >= c.max_paths ? kBridgeFull : children == 0 ? kBridgeExhausted : round == c.max_steps ? kBridgeMaxSteps : children > c.max_live ? kBridgeTooWide : 0;
        if (stop) {
            t[kPairAlive] = 0;
            write_stop(c, p.first_pair + j, stop, found, round, children);
        }
    }
    static_assert(kBridgeFound == kBridgeExpanded + 1, "the two sums lie side by side");
    add_to_counters(c.counters, kBridgeExpanded, sums);
}

__global__ __launch_bounds__(kThreads) void k_bridge_weigh(BridgeCall c, BridgePiece p, uint64_t live, const uint64_t *__restrict__ state) {
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < live; j += uint64_t(gridDim.x) * kThreads) p.weights[j] = weight_of(c, p, state + j * p.words);
}

__global__ __launch_bounds__(kThreads) void k_bridge_scatter(BridgeCall c, BridgePiece p, uint64_t round, uint64_t live, const uint64_t *__restrict__ state,
                                                             const uint64_t *__restrict__ fan_counts, uint64_t *__restrict__ out, uint64_t *__restrict__ queries) {
    const bool left = c.direction == kBridgeLeft;
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < live; j += uint64_t(gridDim.x) * kThreads) {
        const uint64_t *s = state + j * p.words;
        const uint64_t before = p.weights[j], own = weight_of(c, p, s);
        if (j == live - 1) c.counters[kBridgeLive] = (before & 0xffffffffull) + (own & 0xffffffffull);  // the next level
        if (own == 0) continue;
        const uint64_t pair = s[kBridgePair], q = pair - p.first_pair, steps = round - 1, node = s[kBridgeNode], masks = s[kBridgeMasks];
        if (s[kBridgeSteps] != steps || round > c.max_steps) continue;  // (decide flagged it)
        uint64_t slot = before & 0xffffffffull;
        if (own & 0xffffffffull) {  // the children, A < C < G < T
            for (uint32_t sym = 0; sym < 4u; ++sym) {
                if (!(masks >> sym & 1u)) continue;
                if (slot >= p.slots) {
                    atomicOr(c.flags, kFlagInternal);  // (more children than a pair that goes on may have)
                    break;
                }
                uint64_t *o = out + slot * p.words;
                const uint64_t next = next_node(node, sym, c.k, left);
                o[kBridgePair] = pair;
                o[kBridgeNode] = next;
                o[kBridgeSteps] = round;
                o[kBridgeEdgeSum] = s[kBridgeEdgeSum] + fan_counts[4u * j + sym];
                for (uint32_t w = kBridgeMasks; w < kBridgeHeadWords; ++w) o[w] = 0;
                for (uint64_t w = kBridgeHeadWords; w < p.words; ++w) o[w] = s[w];
                o[kBridgeHeadWords + steps / 32u] = s[kBridgeHeadWords + steps / 32u] | uint64_t(sym) << (2u * (steps % 32u));
                write_queries(queries + 4u * slot, next, c.k, left);
                ++slot;
            }
        }
        if (own >> 32) {  // the bridges: numbered from the pair's count before this round, in the order of the frontier
            const uint64_t first = p.table[q * kBridgePairWords + kPairFirst];
            if (first > j) {
                atomicOr(c.flags, kFlagInternal);
                continue;
            }
            uint64_t number = p.table[q * kBridgePairWords + kPairBase] + ((before >> 32) - (first == j ? before >> 32 : p.weights[first] >> 32));
            for (uint32_t sym = 0; sym < 4u; ++sym) {
                if (!(masks >> (4u + sym) & 1u)) continue;
                if (number < c.max_paths) {
                    const uint64_t row = (pair - c.first) * c.max_paths + number;
                    if (c.lengths) c.lengths[row] = round;
                    if (c.edge_sums) c.edge_sums[row] = s[kBridgeEdgeSum] + fan_counts[4u * j + sym];
                    if (c.symbols) {
                        uint8_t *symbols = c.symbols + row * c.max_steps;
                        for (uint64_t i = 0; i < steps; ++i) symbols[i] = code_of(uint32_t(s[kBridgeHeadWords + i / 32u] >> (2u * (i % 32u))) & 3u);
                        symbols[steps] = code_of(sym);
                    }
                }
                ++number;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_bridge_no_seeds(BridgeCall c) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads, at = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    for (uint64_t i = at; i < c.rows; i += stride) write_stop(c, i + c.first, kBridgeNoSeed, 0, 0, 0);
    for (uint64_t e = at; e < c.rows * c.max_paths; e += stride) {
        if (c.lengths) c.lengths[e] = 0;
        if (c.edge_sums) c.edge_sums[e] = 0;
    }
}

}  // namespace

hipError_t launch_bridge_seed(const BridgeCall &c, const BridgePiece &p, uint64_t *state, uint64_t *queries, hipStream_t stream) {
    if (p.pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bridge_seed, dim3(capped_grid(p.pairs * std::max<uint64_t>(c.max_paths, 1), kThreads, kGridCap)), dim3(kThreads), 0, stream, c, p, state, queries);
    return hipGetLastError();
}

hipError_t launch_bridge_start(const BridgeCall &c, const BridgePiece &p, const uint64_t *counts, hipStream_t stream) {
    if (p.pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bridge_start, dim3(capped_grid(p.pairs, kThreads, kGridCap)), dim3(kThreads), 0, stream, c, p, counts);
    return hipGetLastError();
}

hipError_t launch_bridge_decide(const BridgeCall &c, const BridgePiece &p, uint64_t round, uint64_t live, uint64_t *in, const uint64_t *fan_counts, hipStream_t stream) {
    if (live == 0) return hipSuccess;
    const dim3 states(capped_grid(live, kThreads, kGridCap)), pairs(capped_grid(p.pairs, kThreads, kGridCap)), block(kThreads);
    hipLaunchKernelGGL(k_bridge_decide, states, block, 0, stream, c, p, round, live, in, fan_counts);
    hipLaunchKernelGGL(k_bridge_verdict, pairs, block, 0, stream, c, p, round);
    hipLaunchKernelGGL(k_bridge_weigh, states, block, 0, stream, c, p, live, static_cast<const uint64_t *>(in));
    return hipGetLastError();
}

hipError_t launch_bridge_scatter(const BridgeCall &c, const BridgePiece &p, uint64_t round, uint64_t live, const uint64_t *in, const uint64_t *fan_counts, uint64_t *out,
                                 uint64_t *queries, hipStream_t stream) {
    if (live == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bridge_scatter, dim3(capped_grid(live, kThreads, kGridCap)), dim3(kThreads), 0, stream, c, p, round, live, in, fan_counts, out, queries);
    return hipGetLastError();
}

hipError_t launch_bridge_no_seeds(const BridgeCall &c, hipStream_t stream) {
    if (c.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bridge_no_seeds, dim3(capped_grid(c.rows * std::max<uint64_t>(c.max_paths, 1), kThreads, kGridCap)), dim3(kThreads), 0, stream, c);
    return hipGetLastError();
}

}  // namespace msbwt
