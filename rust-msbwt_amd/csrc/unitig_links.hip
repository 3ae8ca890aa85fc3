// gfx950 (MI355X, CDNA4): the kernels of the unitig links (unitig_links.hpp) behind the emission of unitigs.hip -- the degrees of every
// side, their scan into offsets, and the targets.  One thread a slot in the degrees and the targets, eight consecutive words a thread
// and a tile a workgroup in the scan, as in the numbering; no kernel loops on data: a binary search runs the steps the host fixed.
//
// Traffic per emitted unitig: the degrees gather the tail's state and the head's edge byte and scatter two words; the scan streams
// the 2U + 1 words in twice and out once; the targets run one binary search per entry (its first dozen words shared by every thread),
// gather the neighbour's 16-byte state and its head's, and -- canonical, where the neighbour's unitig is not the emitted one of its
// pair -- run a second search for the mirror.  An entry is one 8-byte store at a place only its side's thread writes.
// One writer per plain store: a side's degree and its entries belong to the unitig's one tail or one head; a flag byte gets its bit 1
// from the tail that wrote it in the emission, a kernel earlier on the stream.  Results do not depend on timing.  No MFMA.
#include <hip/hip_runtime.h>

#include "canonical.hpp"
#include "kernels.hpp"
#include "slot_bytes.hpp"
#include "unitig_links.hpp"
#include "unitig_slots.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;
constexpr uint32_t kPerThread = uint32_t(kUnitigTileSlots) / uint32_t(kThreads);
constexpr uint64_t kNoEntry = ~0ull;

template <bool kCanonical>
__device__ __forceinline__ bool own_mirror(const UnitigNodes &g, uint32_t k, uint64_t slot) {
    if constexpr (!kCanonical) return false;
    const uint64_t w = g.kmers[slot];
    return reverse_complement_2bit(w, k) == w;
}

template <bool kCanonical>
__global__ __launch_bounds__(kThreads) void k_link_degrees(UnitigNodes g, const UnitigState *__restrict__ state, const UnitigState *__restrict__ heads, uint32_t k, uint64_t U,
                                                          uint64_t *__restrict__ offsets, uint8_t *__restrict__ out_flags) {
    uint64_t entries[1] = {0};
    if (offsets && blockIdx.x == 0 && threadIdx.x == 0) offsets[2 * U] = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        if (byte_of(g.link_words, i) & kUnitigLinkDown) continue;  // the tails, one a unitig
        const uint64_t head = head_of(g, state, i);
        if (head >= g.n) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        if constexpr (kCanonical)
            if (byte_of(g.link_words, head) & kUnitigSkip) continue;
        const bool mirror = own_mirror<kCanonical>(g, k, head);
        const uint64_t out = uint64_t(__popc(byte_of(g.edge_words, i) >> 4)), in = mirror ? 0u : uint64_t(__popc(byte_of(g.edge_words, head) & 15u));
        if (!offsets) {
            entries[0] += out + in;
            continue;
        }
        const uint64_t u = heads[head].y;
        if (u >= U) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        offsets[2 * u] = out;
        offsets[2 * u + 1] = in;
        if (mirror && out_flags) out_flags[u] |= kUnitigFlagOwnMirror;
    }
    if (!offsets) add_to_counters(g.counters, kUnitigLinkEntries, entries);  // (the same branch in every thread)
}

// ---- the scan of the degrees ----

__device__ __forceinline__ uint64_t tile_thread_sum(const uint64_t *__restrict__ words, uint64_t items, uint64_t t, uint64_t (&mine)[kPerThread]) {
    const uint64_t first = t * kUnitigTileSlots + uint64_t(threadIdx.x) * kPerThread;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPerThread; ++j) {
        mine[j] = first + j < items ? words[first + j] : 0;
        sum += mine[j];
    }
    return sum;
}

__global__ __launch_bounds__(kThreads) void k_link_tile_sums(const uint64_t *__restrict__ words, uint64_t items, TileSums<2> *__restrict__ tiles, uint64_t ntiles) {
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (the same trips for the whole workgroup)
        uint64_t mine[kPerThread];
        const uint64_t v[2] = {tile_thread_sum(words, items, t, mine), 0};  // (k_scan_tile_sums scans two sums a tile at the least)
        const uint64_t s = block_vector_sum(v);
        if (threadIdx.x < 2u) tiles[t].v[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kThreads) void k_link_scan(uint64_t *__restrict__ words, uint64_t items, const TileSums<2> *__restrict__ tiles, uint64_t ntiles) {
    __shared__ uint64_t wave_sums[4];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t mine[kPerThread], all;
        const uint64_t sum = tile_thread_sum(words, items, t, mine);
        uint64_t before = tiles[t].v[0] + block_exclusive_sum(sum, wave_sums, &all);
        const uint64_t first = t * kUnitigTileSlots + uint64_t(threadIdx.x) * kPerThread;
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; ++j) {
            if (first + j < items) words[first + j] = before;  // (a thread writes the words it read)
            before += mine[j];
        }
    }
}

// ---- the targets ----

struct LinkView {
    const UnitigState *state, *heads;
    uint32_t k, probes;
    uint64_t U;
};

// the number of the unitig that starts at `head`, or U where there is none
__device__ __forceinline__ uint64_t number_of(const LinkView &v, uint64_t head) {
    const uint64_t u = v.heads[head].y;
    return u < v.U ? u : v.U;
}

// The entry for the node of word w, which lies at an end of an emitted unitig v or of the mirror of one.  leaving == false: w is the
// node an out-edge of a last node reaches, so it is a first node -- 2v where its unitig is emitted, else 2v + 1 with v the unitig of
// rc(w), which is a last node.  leaving == true: w is the node an in-edge of a first node comes from, a last node, and the entry is the
// one that reaches rc(w) -- 2v + 1 where the unitig of w is emitted (2v where it is its own mirror), else 2v with v the unitig that
// starts at rc(w).  kNoEntry where the arrays do not say so.
template <bool kCanonical>
__device__ __forceinline__ uint64_t entry_of(const UnitigNodes &g, const LinkView &v, uint64_t w, bool leaving) {
    const uint64_t slot = slot_of(g.kmers, g.n, v.probes, w);
    if (slot >= g.n) return kNoEntry;
    const uint64_t head = head_of(g, v.state, slot);
    if (head >= g.n || (!leaving && head != slot)) return kNoEntry;
    bool emitted = true;
    if constexpr (kCanonical) emitted = !(byte_of(g.link_words, head) & kUnitigSkip);
    if (emitted) {
        const uint64_t u = number_of(v, head);
        if (u >= v.U) return kNoEntry;
        return 2 * u + (leaving && !own_mirror<kCanonical>(g, v.k, head) ? 1u : 0u);
    }
    if constexpr (kCanonical) {
        const uint64_t mirror = slot_of(g.kmers, g.n, v.probes, reverse_complement_2bit(w, v.k));
        if (mirror >= g.n) return kNoEntry;
        const uint64_t mirror_head = head_of(g, v.state, mirror);
        if (mirror_head >= g.n || (leaving && mirror_head != mirror) || (byte_of(g.link_words, mirror_head) & kUnitigSkip)) return kNoEntry;
        const uint64_t u = number_of(v, mirror_head);
        if (u >= v.U) return kNoEntry;
        return 2 * u + (leaving ? 0u : 1u);
    }
    return kNoEntry;
}

template <bool kCanonical>
__global__ __launch_bounds__(kThreads) void k_link_targets(UnitigNodes g, LinkView v, uint64_t L, const uint64_t *__restrict__ offsets, uint64_t *__restrict__ targets) {
    const uint64_t mask = ~0ull >> (64u - 2u * v.k);
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        const bool tail = !(byte_of(g.link_words, i) & kUnitigLinkDown);
        const uint64_t head = head_of(g, v.state, i);
        if (head >= g.n) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        if (!tail && head != i) continue;
        if constexpr (kCanonical)
            if (byte_of(g.link_words, head) & kUnitigSkip) continue;
        const uint64_t u = number_of(v, head);
        if (u >= v.U) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        const uint64_t word = g.kmers[i];
        const uint32_t edges = byte_of(g.edge_words, i);
        bool broken = false;
        if (tail) {  // side 2u: the successors, A C G T
            const uint32_t out = edges >> 4;
            uint64_t at = offsets[2 * u];
            const uint64_t end = offsets[2 * u + 1];
            if (at > end || end > L || end - at != uint64_t(__popc(out))) {
                broken = true;
            } else {
#pragma unroll
                for (uint32_t c = 0; c < 4u; ++c) {
                    if (!(out & (1u << c))) continue;
                    const uint64_t e = entry_of<kCanonical>(g, v, ((word << 2) & mask) | c, false);
                    if (e == kNoEntry) broken = true;
                    else targets[at] = e;
                    ++at;
                }
            }
        }
        if (head == i && !own_mirror<kCanonical>(g, v.k, i)) {  // side 2u + 1: the predecessors T G C A, whose complements lead out of rc(u)
            const uint32_t in = edges & 15u;
            uint64_t at = offsets[2 * u + 1];
            const uint64_t end = offsets[2 * u + 2];  // (u < U: a word of the offsets)
            if (at > end || end > L || end - at != uint64_t(__popc(in))) {
                broken = true;
            } else {
#pragma unroll
                for (uint32_t c = 0; c < 4u; ++c) {
                    const uint64_t j = 3u - c;
                    if (!(in & (1u << j))) continue;
                    const uint64_t e = entry_of<kCanonical>(g, v, (j << (2u * (v.k - 1u))) | (word >> 2), true);
                    if (e == kNoEntry) broken = true;
                    else targets[at] = e;
                    ++at;
                }
            }
        }
        if (broken) atomicOr(g.flags, kFlagInternal);
    }
}

bool usable(const UnitigNodes &g) { return g.kmers && g.edge_words && g.link_words && g.counters && g.flags; }
dim3 slots_grid(const UnitigNodes &g) { return dim3(capped_grid(g.n, uint64_t(kThreads), kGridCap)); }

}  // namespace

hipError_t launch_unitig_link_degrees(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, bool canonical, uint64_t U, uint64_t *offsets,
                                      uint8_t *out_flags, hipStream_t stream) {
    if (!usable(g) || !state || (offsets && !heads) || k < 1 || k > (canonical ? 31u : 32u)) return hipErrorInvalidValue;
    if (g.n == 0) {
        if (offsets) return hipMemsetAsync(offsets, 0, 8 * unitig_link_sides(U), stream);
        return hipSuccess;
    }
    if (canonical)
        hipLaunchKernelGGL(k_link_degrees<true>, slots_grid(g), dim3(kThreads), 0, stream, g, state, heads, k, U, offsets, out_flags);
    else
        hipLaunchKernelGGL(k_link_degrees<false>, slots_grid(g), dim3(kThreads), 0, stream, g, state, heads, k, U, offsets, out_flags);
    return hipGetLastError();
}

hipError_t launch_unitig_link_scan(uint64_t U, uint64_t *offsets, void *tiles, hipStream_t stream) {
    static_assert(sizeof(TileSums<2>) == kUnitigTileBytes && kPerThread * kThreads == kUnitigTileSlots, "a tile");
    if (!offsets || !tiles) return hipErrorInvalidValue;
    const uint64_t items = unitig_link_sides(U), ntiles = unitig_tiles(items);
    TileSums<2> *sums = static_cast<TileSums<2> *>(tiles);
    const dim3 grid(capped_grid(ntiles, 1, kGridCap));
    hipLaunchKernelGGL(k_link_tile_sums, grid, dim3(kThreads), 0, stream, offsets, items, sums, ntiles);
    hipLaunchKernelGGL(k_scan_tile_sums<2>, dim3(1), dim3(1024), 0, stream, sums, ntiles, static_cast<uint64_t *>(nullptr));
    hipLaunchKernelGGL(k_link_scan, grid, dim3(kThreads), 0, stream, offsets, items, sums, ntiles);
    return hipGetLastError();
}

hipError_t launch_unitig_link_targets(const UnitigNodes &g, const UnitigState *state, const UnitigState *heads, uint32_t k, bool canonical, uint32_t probes, uint64_t U,
                                      uint64_t L, const uint64_t *offsets, uint64_t *targets, hipStream_t stream) {
    if (!usable(g) || !state || !heads || !offsets || (L && !targets) || k < 1 || k > (canonical ? 31u : 32u)) return hipErrorInvalidValue;
    if (g.n == 0 || L == 0) return hipSuccess;
    const LinkView v{state, heads, k, probes, U};
    if (canonical)
        hipLaunchKernelGGL(k_link_targets<true>, slots_grid(g), dim3(kThreads), 0, stream, g, v, L, offsets, targets);
    else
        hipLaunchKernelGGL(k_link_targets<false>, slots_grid(g), dim3(kThreads), 0, stream, g, v, L, offsets, targets);
    return hipGetLastError();
}

}  // namespace msbwt
