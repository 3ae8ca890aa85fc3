// gfx950 (MI355X, CDNA4): the kernels of the canonical unitigs (canonical_unitigs.hpp) around the compaction of unitigs.hip: doubling
// the classes into nodes, the (k+1)-mer words of a chunk, the fold of their counts into edge bytes, the cuts after the links and the
// choice between a unitig and its mirror.  (The sort that puts the nodes in word order between the doubling and the edges is
// radix_sort.hip's.)  One thread a slot everywhere; no kernel loops on data.
//
// Traffic per node: the doubling streams 24 bytes a class in and 16 bytes a node out; the fold reads the node's word and four
// counts, runs one binary search for its successors (they are neighbours in word order) and one per successor for the mirrored
// edge's count, and ORs bits as the edge pass does; the cut gathers one word; the choice runs one search per tail.  A binary search
// reads ceil(log2 N) + 1 words, the first dozen of which every thread shares.
// One writer per plain store: keys, payloads and states at the thread's own slot or at a reserved one; pred[j] as in kmer_graph.hip
// (read only where the node has ONE in-edge, which has one writer); edge and link bits by vector atomics.  No MFMA.
#include <hip/hip_runtime.h>

#include "canonical.hpp"
#include "canonical_unitigs.hpp"
#include "kernels.hpp"
#include "slot_bytes.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGridCap = 256u * 8u;

// the first slot whose word is not below w (N: none); at most 41 halvings, N < 2^41
__device__ __forceinline__ uint64_t lower_bound(const uint64_t *__restrict__ keys, uint64_t N, uint64_t w) {
    uint64_t lo = 0, hi = N;
    for (uint32_t step = 0; step < 41u && lo < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the slot of w, or N where w is no node
__device__ __forceinline__ uint64_t slot_of(const uint64_t *__restrict__ keys, uint64_t N, uint64_t w) {
    const uint64_t lo = lower_bound(keys, N, w);
    return lo < N && keys[lo] == w ? lo : N;
}

__global__ __launch_bounds__(kThreads) void k_double(const uint64_t *__restrict__ words, const uint64_t *__restrict__ own, const uint64_t *__restrict__ other, uint64_t n,
                                                    uint32_t k, uint64_t *__restrict__ keys, uint64_t *__restrict__ vals, unsigned long long *__restrict__ counters,
                                                    uint32_t *__restrict__ flags) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < n; base += uint64_t(gridDim.x) * kThreads) {  // (the same trips for the whole wave)
        const uint64_t i = base + threadIdx.x;
        uint64_t w = 0, r = 0, count = 0;
        if (i < n) {
            w = words[i];
            r = reverse_complement_2bit(w, k);
            count = own[i] + other[i];
            keys[i] = w;
            vals[i] = count;
        }
        const bool second = i < n && r != w;
        const uint64_t peers = __ballot(second);
        if (!peers) continue;
        const uint32_t leader = uint32_t(__ffsll((unsigned long long)peers) - 1);
        unsigned long long start = 0;
        if (lane == leader) start = atomicAdd(counters + kCanonicalUnitigSeconds, (unsigned long long)__popcll(peers));
        start = __shfl(start, int(leader));
        if (second) {
            const uint64_t at = start + uint64_t(__popcll(peers & ((1ull << lane) - 1ull)));
            if (at >= n) {  // (a class has one second member at the most)
                atomicOr(flags, kFlagInternal);
            } else {
                keys[n + at] = r;
                vals[n + at] = count;
            }
        }
    }
}

// ---- edges ----

__global__ __launch_bounds__(kThreads) void k_edge_words(const uint64_t *__restrict__ keys, uint64_t first, uint64_t m, uint64_t *__restrict__ out) {
    for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < m; j += uint64_t(gridDim.x) * kThreads) {
        const uint64_t e = keys[first + j] << 2;  // (k <= 31: 2k + 2 bits)
        ulonglong2 *to = reinterpret_cast<ulonglong2 *>(out + 4 * j);
        to[0] = ulonglong2{e, e | 1ull};
        to[1] = ulonglong2{e | 2ull, e | 3ull};
    }
}

__global__ __launch_bounds__(kThreads) void k_fold(const uint64_t *__restrict__ keys, uint64_t N, uint32_t k, uint64_t min_edge, const uint64_t *__restrict__ cnt,
                                                  uint32_t *__restrict__ edge_words, uint64_t *__restrict__ pred, unsigned long long *__restrict__ counters,
                                                  uint32_t *__restrict__ flags) {
    const uint64_t mask = ~0ull >> (64u - 2u * k);
    uint64_t hairpins[1] = {0};
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < N; i += uint64_t(gridDim.x) * kThreads) {
        const uint64_t q = keys[i], first_symbol = q >> (2u * (k - 1u)), base = (q << 2) & mask;
        uint64_t at = lower_bound(keys, N, base);  // the successors that are nodes follow each other from here
        uint32_t out = 0;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            if (at >= N || keys[at] != (base | c)) continue;  // q[1:].c is no node: no edge, whatever the count
            const uint64_t j = at++, e = (q << 2) | c;
            uint64_t cc = cnt[4 * i + c];
            const bool hairpin = reverse_complement_2bit(e, k + 1u) == e;
            if (!hairpin) {  // rc(q.c) = rc(q').(3 - q0): the out-edge 3 - q0 of q' mirror
                const uint64_t p = slot_of(keys, N, reverse_complement_2bit(keys[j], k));
                if (p >= N) {  // (D is closed under rc)
                    atomicOr(flags, kFlagInternal);
                    continue;
                }
                cc += cnt[4 * p + (3u - first_symbol)];
            }
            if (cc < min_edge) continue;
            out |= 16u << c;
            or_slot_bits(edge_words, j, 1u << uint32_t(first_symbol));
            pred[j] = i;
            hairpins[0] += hairpin ? 1u : 0u;
        }
        if (out) or_slot_bits(edge_words, i, out);
    }
    add_to_counters(counters, kCanonicalUnitigHairpins, hairpins);
}

// ---- cuts and choice ----

__global__ __launch_bounds__(kThreads) void k_cut(UnitigNodes g, uint32_t k, UnitigState *__restrict__ state, unsigned long long *__restrict__ counters) {
    uint64_t cut[1] = {0};
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < g.n; i += uint64_t(gridDim.x) * kThreads) {
        if (!(byte_of(g.link_words, i) & kUnitigLinkUp)) continue;
        const uint64_t p = g.pred[i];
        if (p >= g.n) {  // (launch_unitig_links linked up over a slot)
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        const uint64_t w = g.kmers[i], wp = g.kmers[p], r = reverse_complement_2bit(w, k);
        if (r != w && r != wp && reverse_complement_2bit(wp, k) != wp) continue;
        clear_slot_bits(g.link_words, i, kUnitigLinkUp);
        clear_slot_bits(g.link_words, p, kUnitigLinkDown);
        state[i] = UnitigState{i, kUnitigDone};
        cut[0] += 1;
    }
    const uint64_t s = add_to_counters(counters, kCanonicalUnitigCut, cut);
    if (threadIdx.x == 0 && s) {
        atomicAdd(g.counters + kUnitigLinks, 0ull - (unsigned long long)s);  // (every cut link was counted, and its node as unfinished)
        atomicAdd(g.counters + kUnitigUnfinished, 0ull - (unsigned long long)s);
    }
}

__global__ __launch_bounds__(kThreads) void k_choose(UnitigNodes g, uint32_t k, const UnitigState *__restrict__ state, unsigned long long *__restrict__ counters) {
    uint64_t sums[3] = {0, 0, 0};  // emitted unitigs, their nodes, the circular ones: kCanonicalUnitigEmitted ..
    for (uint64_t t = uint64_t(blockIdx.x) * kThreads + threadIdx.x; t < g.n; t += uint64_t(gridDim.x) * kThreads) {
        if (byte_of(g.link_words, t) & kUnitigLinkDown) continue;
        const UnitigState s = state[t];
        const uint64_t mirror = slot_of(g.kmers, g.n, reverse_complement_2bit(g.kmers[t], k));
        if (!(s.y & kUnitigDone) || s.x >= g.n || mirror >= g.n) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        const UnitigState m = state[mirror];  // the mirror of a tail is the first node of the mirror path, and some node of the mirror cycle
        if (!(m.y & kUnitigDone) || m.x >= g.n) {
            atomicOr(g.flags, kFlagInternal);
            continue;
        }
        if (s.x > m.x) {
            or_slot_bits(g.link_words, s.x, kUnitigSkip);
        } else {
            sums[0] += 1;
            sums[1] += (s.y & kDistance) + 1ull;
            sums[2] += (byte_of(g.link_words, s.x) & kUnitigOnCycle) ? 1u : 0u;
        }
    }
    add_to_counters(counters, kCanonicalUnitigEmitted, sums);
}

dim3 grid_for(uint64_t items) { return dim3(capped_grid(items, uint64_t(kThreads), kGridCap)); }

}  // namespace

hipError_t launch_canonical_unitig_double(const uint64_t *words, const uint64_t *own, const uint64_t *other, uint64_t n, uint32_t k, uint64_t *keys, uint64_t *vals,
                                          unsigned long long *counters, uint32_t *flags, hipStream_t stream) {
    if (!words || !own || !other || !keys || !vals || !counters || !flags || k < 1 || k > 31) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_double, grid_for(n), dim3(kThreads), 0, stream, words, own, other, n, k, keys, vals, counters, flags);
    return hipGetLastError();
}

hipError_t launch_canonical_unitig_edge_words(const uint64_t *keys, uint64_t first, uint64_t m, uint64_t *out, hipStream_t stream) {
    if (!keys || !out || (reinterpret_cast<uintptr_t>(out) & 15u)) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_edge_words, grid_for(m), dim3(kThreads), 0, stream, keys, first, m, out);
    return hipGetLastError();
}

hipError_t launch_canonical_unitig_fold(const uint64_t *keys, uint64_t N, uint32_t k, uint64_t min_edge, const uint64_t *cnt, uint32_t *edge_words, uint64_t *pred,
                                        unsigned long long *counters, uint32_t *flags, hipStream_t stream) {
    if (!keys || !cnt || !edge_words || !pred || !counters || !flags || k < 1 || k > 31 || min_edge < 1) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fold, grid_for(N), dim3(kThreads), 0, stream, keys, N, k, min_edge, cnt, edge_words, pred, counters, flags);
    return hipGetLastError();
}

hipError_t launch_canonical_unitig_cut(const UnitigNodes &g, uint32_t k, UnitigState *state, unsigned long long *counters, hipStream_t stream) {
    if (!g.kmers || !g.pred || !g.link_words || !g.counters || !g.flags || !state || !counters || k < 1 || k > 31) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cut, grid_for(g.n), dim3(kThreads), 0, stream, g, k, state, counters);
    return hipGetLastError();
}

hipError_t launch_canonical_unitig_choose(const UnitigNodes &g, uint32_t k, const UnitigState *state, unsigned long long *counters, hipStream_t stream) {
    if (!g.kmers || !g.link_words || !g.flags || !state || !counters || k < 1 || k > 31) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_choose, grid_for(g.n), dim3(kThreads), 0, stream, g, k, state, counters);
    return hipGetLastError();
}

}  // namespace msbwt
