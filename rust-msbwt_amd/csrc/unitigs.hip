// gfx950 (MI355X, CDNA4): the kernels that compact the k-mer graph into unitigs (unitigs.hpp) -- links, pointer jumping, cycle opening,
// numbering and the emission of sequences -- over the n slots of the sorted dump.  Every kernel strides over the slots with one
// thread a slot (the numbering: eight consecutive slots a thread, a tile a workgroup), and none loops on data: the rounds are the host's.
//
// Traffic per node: the links read the edge byte and, where in = 1, gather the predecessor's (8 + 4 bytes); a jumping round reads and
// writes the node's own 16-byte state in order and, while the node is unfinished, gathers one 16-byte state; the emission gathers the
// head's 16 bytes and scatters one symbol byte, and adds the count to its unitig's sum with one 64-bit atomic.
// Two writers never meet in a plain store: a state, a heads[] entry, an ends byte and a flag have one writer each (the node itself,
// the unitig's one tail); link bytes share 32-bit words and are set and cleared by vector atomics, as the edge bytes are.
// Results do not depend on timing: a round reads one buffer and writes the other, and integer sums and maxima commute.  No MFMA.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "slot_bytes.hpp"
#include "unitigs.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;
constexpr uint32_t kPerThread = uint32_t(kUnitigTileSlots) / uint32_t(kThreads);

// A C G T (0..3) -> the library's symbol codes 1 2 3 5
__device__ __forceinline__ uint8_t code_of(uint64_t two_bits) { return uint8_t(two_bits == 3u ? 5u : two_bits + 1u); }

__global__ __launch_bounds__(kThreads) void k_unitig_links(UnitigNodes g, UnitigState *__restrict__ state) {
    uint64_t sums[3] = {0, 0, 0}, unfinished[1] = {0};  // edges, links, circular: kUnitigEdges ..
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        const uint32_t in = uint32_t(__popc(byte_of(g.edge_words, i) & 15u));
        sums[0] += in;
        UnitigState s{i, kUnitigDone};
        if (in == 1u) {
            const uint64_t p = g.pred[i];
            if (p >= g.n) {  // (the edge pass wrote a slot for every in-edge)
                atomicOr(g.flags, kFlagInternal);
            } else if (__popc(byte_of(g.edge_words, p) >> 4) == 1) {
                sums[1] += 1;
                if (p == i) {  // A^k with A^(k+1) and nothing else: a cycle of one
                    or_slot_bits(g.link_words, i, kUnitigOnCycle);
                    sums[2] += 1;
                } else {
                    or_slot_bits(g.link_words, i, kUnitigLinkUp);
                    or_slot_bits(g.link_words, p, kUnitigLinkDown);
                    s = UnitigState{p, 1ull};
                    unfinished[0] += 1;
                }
            }
        }
        state[i] = s;
    }
    add_to_counters(g.counters, kUnitigEdges, sums);
    add_to_counters(g.counters, kUnitigUnfinished, unfinished);
}

// kMin: the min-label rounds of the cycles; else the ranking
template <bool kMin>
__global__ __launch_bounds__(kThreads) void k_unitig_jump(UnitigNodes g, const UnitigState *__restrict__ src, UnitigState *__restrict__ dst) {
    uint64_t unfinished[1] = {0};
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        UnitigState s = src[i];
        if (!(s.y & kUnitigDone)) {
            if (s.x >= g.n) {  // (an ancestor is a slot)
                atomicOr(g.flags, kFlagInternal);
            } else {
                const UnitigState a = src[s.x];
                s.x = a.x;
                if constexpr (kMin)
                    s.y = s.y < a.y ? s.y : a.y;  // (an unfinished node's ancestors are unfinished: labels, no done bit)
                else
                    s.y = (s.y + (a.y & kDistance)) | (a.y & kUnitigDone);
            }
            if (!(s.y & kUnitigDone)) unfinished[0] += 1;
        }
        dst[i] = s;
    }
    if constexpr (!kMin) add_to_counters(g.counters, kUnitigUnfinished, unfinished);
}

__global__ __launch_bounds__(kThreads) void k_unitig_cycle_seed(UnitigNodes g, UnitigState *__restrict__ state) {
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads)
        if (!(state[i].y & kUnitigDone)) state[i] = UnitigState{g.pred[i], i};  // (linked up: pred[i] < n was checked)
}

__global__ __launch_bounds__(kThreads) void k_unitig_cycle_cut(UnitigNodes g, UnitigState *__restrict__ state) {
    uint64_t circular[1] = {0}, unfinished[1] = {0};
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        const UnitigState s = state[i];
        if (s.y & kUnitigDone) continue;
        const uint64_t p = g.pred[i];
        if (s.y > i || p >= g.n) {  // (the smallest slot of a cycle is at most one's own)
            atomicOr(g.flags, kFlagInternal);
        } else if (s.y == i) {
            clear_slot_bits(g.link_words, i, kUnitigLinkUp);
            clear_slot_bits(g.link_words, p, kUnitigLinkDown);
            or_slot_bits(g.link_words, i, kUnitigOnCycle);
            state[i] = UnitigState{i, kUnitigDone};
            circular[0] += 1;
        } else {
            state[i] = UnitigState{p, 1ull};
            unfinished[0] += 1;
        }
    }
    add_to_counters(g.counters, kUnitigCircular, circular);
    add_to_counters(g.counters, kUnitigUnfinished, unfinished);
}

__global__ __launch_bounds__(kThreads) void k_unitig_tails(UnitigNodes g, const UnitigState *__restrict__ state, UnitigState *__restrict__ heads) {
    unsigned long long longest = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        if (byte_of(g.link_words, i) & kUnitigLinkDown) continue;
        const UnitigState s = state[i];
        if (!(s.y & kUnitigDone) || s.x >= g.n) {  // (the host ranks until nothing is unfinished)
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        const unsigned long long nodes = (s.y & kDistance) + 1ull;
        heads[s.x].x = nodes;
        longest = nodes > longest ? nodes : longest;
    }
    longest = wave_max(longest);
    if ((threadIdx.x & 63u) == 0u && longest) atomicMax(g.counters + kUnitigLongest, longest);
}

// what a thread's eight slots of tile t hold: heads, and the nodes of the unitigs that start at them
__device__ __forceinline__ void tile_thread_sums(const UnitigNodes &g, const UnitigState *__restrict__ heads, uint64_t t, uint64_t (&v)[2]) {
    v[0] = v[1] = 0;
    const uint64_t first = t * kUnitigTileSlots + uint64_t(threadIdx.x) * kPerThread;
#pragma unroll
    for (uint32_t j = 0; j < kPerThread; ++j) {
        const uint64_t i = first + j;
        if (i < g.n && !(byte_of(g.link_words, i) & (kUnitigLinkUp | kUnitigSkip))) {
            v[0] += 1;
            v[1] += heads[i].x;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_unitig_tile_sums(UnitigNodes g, const UnitigState *__restrict__ heads, TileSums<2> *__restrict__ tiles, uint64_t ntiles) {
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (the same trips for the whole workgroup)
        uint64_t v[2];
        tile_thread_sums(g, heads, t, v);
        const uint64_t s = block_vector_sum(v);
        if (threadIdx.x < 2u) tiles[t].v[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kThreads) void k_unitig_number(UnitigNodes g, UnitigState *__restrict__ heads, const TileSums<2> *__restrict__ tiles, uint64_t ntiles, uint32_t k,
                                                           uint64_t U, uint64_t S, uint64_t *__restrict__ offsets) {
    __shared__ uint64_t wave_sums[4];
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[U] = S;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t v[2], all;
        tile_thread_sums(g, heads, t, v);
        uint64_t number = tiles[t].v[0] + block_exclusive_sum(v[0], wave_sums, &all);
        uint64_t before = tiles[t].v[1] + block_exclusive_sum(v[1], wave_sums, &all);
        const uint64_t first = t * kUnitigTileSlots + uint64_t(threadIdx.x) * kPerThread;
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; ++j) {
            const uint64_t i = first + j;
            if (i >= g.n || (byte_of(g.link_words, i) & (kUnitigLinkUp | kUnitigSkip))) continue;
            const uint64_t nodes = heads[i].x;
            if (number >= U || before + number * (k - 1u) >= S) {  // (U and S are what the counters said)
                atomicOr(g.flags, kFlagInternal);
                heads[i] = UnitigState{0ull, U};  // (no node of it emits)
            } else {
                heads[i] = UnitigState{before, number};
                offsets[number] = before + number * (k - 1u);
            }
            number += 1;
            before += nodes;
        }
    }
}

// kSkip: the nodes of a unitig whose head carries kUnitigSkip emit nothing (canonical_unitigs.hpp; the plain call sets no such bit)
template <bool kSkip>
__global__ __launch_bounds__(kThreads) void k_unitig_emit(UnitigNodes g, const UnitigState *__restrict__ state, const UnitigState *__restrict__ heads, uint32_t k, uint64_t U,
                                                         uint64_t S, uint8_t *__restrict__ symbols, unsigned long long *__restrict__ count_sums, uint8_t *__restrict__ ends,
                                                         uint8_t *__restrict__ out_flags) {
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        const UnitigState s = state[i];
        const uint64_t head = s.x, distance = s.y & kDistance;
        if (!(s.y & kUnitigDone) || head >= g.n) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        if constexpr (kSkip)
            if (byte_of(g.link_words, head) & kUnitigSkip) continue;
        const UnitigState h = heads[head];
        const uint64_t u = h.y, offset = h.x + u * (k - 1u), at = offset + (k - 1u) + distance;
        if (u >= U || at >= S) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        const uint64_t word = g.kmers[i];
        if (symbols) {
            symbols[at] = code_of(word & 3u);
            if (distance == 0u)  // the head: its first k - 1 symbols end below `at`
                for (uint32_t j = 0; j + 1u < k; ++j) symbols[offset + j] = code_of((word >> (2u * (k - 1u - j))) & 3u);
        }
        if (count_sums) atomicAdd(count_sums + u, (unsigned long long)g.counts[i]);
        if (!(byte_of(g.link_words, i) & kUnitigLinkDown)) {  // the tail, one a unitig
            if (ends) ends[u] = uint8_t((byte_of(g.edge_words, head) & 0x0Fu) | (byte_of(g.edge_words, i) & 0xF0u));
            if (out_flags) out_flags[u] = (byte_of(g.link_words, head) & kUnitigOnCycle) ? 1u : 0u;
        }
    }
}

bool usable(const UnitigNodes &g) { return g.kmers && g.counts && g.pred && g.edge_words && g.link_words && g.counters && g.flags; }
dim3 slots_grid(const UnitigNodes &g) { return dim3(capped_grid(g.n, uint64_t(kThreads), kGridCap)); }

}  // namespace

hipError_t launch_unitig_links(const UnitigNodes &g, UnitigState *state, hipStream_t stream) {
    if (!usable(g) || !state) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unitig_links, slots_grid(g), dim3(kThreads), 0, stream, g, state);
    return hipGetLastError();
}

hipError_t launch_unitig_jump(const UnitigNodes &g, const UnitigState *src, UnitigState *dst, hipStream_t stream) {
    if (!usable(g) || !src || !dst || src == dst) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unitig_jump<false>, slots_grid(g), dim3(kThreads), 0, stream, g, src, dst);
    return hipGetLastError();
}

hipError_t launch_unitig_cycle_seed(const UnitigNodes &g, UnitigState *state, hipStream_t stream) {
    if (!usable(g) || !state) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unitig_cycle_seed, slots_grid(g), dim3(kThreads), 0, stream, g, state);
    return hipGetLastError();
}

hipError_t launch_unitig_cycle_jump(const UnitigNodes &g, const UnitigState *src, UnitigState *dst, hipStream_t stream) {
    if (!usable(g) || !src || !dst || src == dst) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unitig_jump<true>, slots_grid(g), dim3(kThreads), 0, stream, g, src, dst);
    return hipGetLastError();
}

hipError_t launch_unitig_cycle_cut(const UnitigNodes &g, UnitigState *state, hipStream_t stream) {
    if (!usable(g) || !state) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unitig_cycle_cut, slots_grid(g), dim3(kThreads), 0, stream, g, state);
    return hipGetLastError();
}

hipError_t launch_unitig_tails(const UnitigNodes &g, const UnitigState *state, UnitigState *heads, hipStream_t stream) {
    if (!usable(g) || !state || !heads || state == heads) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unitig_tails, slots_grid(g), dim3(kThreads), 0, stream, g, state, heads);
    return hipGetLastError();
}

hipError_t launch_unitig_number(const UnitigNodes &g, UnitigState *heads, void *tiles, uint32_t k, uint64_t U, uint64_t S, uint64_t *offsets, hipStream_t stream) {
    static_assert(sizeof(TileSums<2>) == kUnitigTileBytes && kPerThread * kThreads == kUnitigTileSlots, "a tile");
    if (!usable(g) || !heads || !tiles || !offsets || k < 1) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    const uint64_t ntiles = unitig_tiles(g.n);
    TileSums<2> *sums = static_cast<TileSums<2> *>(tiles);
    const dim3 grid(capped_grid(ntiles, 1, kGridCap));
    hipLaunchKernelGGL(k_unitig_tile_sums, grid, dim3(kThreads), 0, stream, g, heads, sums, ntiles);
    hipLaunchKernelGGL(k_scan_tile_sums<2>, dim3(1), dim3(1024), 0, stream, sums, ntiles, static_cast<uint64_t *>(nullptr));
    hipLaunchKernelGGL(k_unitig_number, grid, dim3(kThreads), 0, stream, g, heads, sums, ntiles, k, U, S, offsets);
    return hipGetLastError();
}

hipError_t launch_unitig_emit(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, uint64_t U, uint64_t S, uint8_t *symbols,
                              uint64_t *count_sums, uint8_t *ends, uint8_t *out_flags, hipStream_t stream, bool skip_marked) {
    if (!usable(g) || !state || !heads || k < 1) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(count_sums);
    if (skip_marked)
        hipLaunchKernelGGL(k_unitig_emit<true>, slots_grid(g), dim3(kThreads), 0, stream, g, state, heads, k, U, S, symbols, sums, ends, out_flags);
    else
        hipLaunchKernelGGL(k_unitig_emit<false>, slots_grid(g), dim3(kThreads), 0, stream, g, state, heads, k, U, S, symbols, sums, ends, out_flags);
    return hipGetLastError();
}

}  // namespace msbwt
