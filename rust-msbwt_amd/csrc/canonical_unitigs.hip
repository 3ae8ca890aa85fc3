// gfx950 (MI355X, CDNA4): the kernels of the canonical unitigs (canonical_unitigs.hpp) around the compaction of unitigs.hip: doubling
// the classes into nodes, the radix passes that put the nodes in word order, the (k+1)-mer words of a chunk, the fold of their counts
// into edge bytes, the cuts after the links and the choice between a unitig and its mirror.  One thread a slot everywhere but in the
// sort (a tile of 4096 keys a workgroup, as in reads_build.hip, whose pass this is with a 64-bit payload); no kernel loops on data.
//
// Traffic per node: the doubling streams 24 bytes a class in and 16 bytes a node out; a radix pass reads the keys twice and moves 16
// bytes; the fold reads the node's word and four counts, runs one binary search for its successors (they are neighbours in word
// order) and one per successor for the mirrored edge's count, and ORs bits as the edge pass does; the cut gathers one word; the choice
// runs one search per tail.  A binary search reads ceil(log2 N) + 1 words, the first dozen of which every thread shares.
// One writer per plain store: keys, payloads and states at the thread's own slot or at a reserved one; pred[j] as in kmer_graph.hip
// (read only where the node has ONE in-edge, which has one writer); edge and link bits by vector atomics.  No MFMA.
#include <hip/hip_runtime.h>

#include "canonical.hpp"
#include "canonical_unitigs.hpp"
#include "kernels.hpp"
#include "run_encode.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kGridCap = 256u * 8u;
constexpr uint32_t kRounds = uint32_t(kCanonicalUnitigSortTile) / uint32_t(kThreads);
constexpr uint32_t kDigitBits = 8, kDigits = 1u << kDigitBits;
constexpr unsigned long long kDistance = ~kUnitigDone;
static_assert(kDigits == uint32_t(kThreads) && kRounds * kThreads == kCanonicalUnitigSortTile, "one thread per digit when a tile's counts are laid out");

__device__ __forceinline__ uint32_t byte_of(const uint32_t *__restrict__ words, uint64_t slot) { return (words[slot >> 2] >> (8u * (uint32_t(slot) & 3u))) & 0xFFu; }
__device__ __forceinline__ void or_bits(uint32_t *__restrict__ words, uint64_t slot, uint32_t bits) { atomicOr(words + (slot >> 2), bits << (8u * (uint32_t(slot) & 3u))); }
__device__ __forceinline__ void clear_bits(uint32_t *__restrict__ words, uint64_t slot, uint32_t bits) { atomicAnd(words + (slot >> 2), ~(bits << (8u * (uint32_t(slot) & 3u)))); }

// counters[at + j] += the workgroup's sum of v[j]; the whole workgroup calls it
template <uint32_t N>
__device__ __forceinline__ void add_to_counters(unsigned long long *__restrict__ counters, uint32_t at, const uint64_t (&v)[N]) {
    const uint64_t s = block_vector_sum(v);
    if (threadIdx.x < N && s) atomicAdd(counters + at + threadIdx.x, (unsigned long long)s);
}

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

// ---- one stable radix pass: tile t = elements [t * kCanonicalUnitigSortTile, ...) ----

// hist[digit * ntiles + tile] = the tile's elements with that digit
__global__ __launch_bounds__(kThreads) void k_sort_histogram(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift, uint64_t ntiles, uint64_t *__restrict__ hist) {
    __shared__ uint32_t counts[kDigits];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (the same trips for the whole workgroup)
        counts[threadIdx.x] = 0u;
        __syncthreads();
        const uint64_t base = t * kCanonicalUnitigSortTile;
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint64_t i = base + r * kThreads + threadIdx.x;
            if (i < n) atomicAdd(&counts[uint32_t(keys[i] >> shift) & (kDigits - 1u)], 1u);
        }
        __syncthreads();
        hist[uint64_t(threadIdx.x) * ntiles + t] = counts[threadIdx.x];
        __syncthreads();
    }
}

// hist: scanned.  A wave takes kRounds rows of 64 consecutive elements; a lane's rank among the tile's elements of its digit is
// (what earlier waves hold) + (what the wave's earlier rows hold) + (the lanes before it in its row with the same digit).
__global__ __launch_bounds__(kThreads) void k_sort_scatter(const uint64_t *__restrict__ keys_in, const uint64_t *__restrict__ vals_in, uint64_t n, uint32_t shift,
                                                          uint64_t ntiles, const uint64_t *__restrict__ hist, uint64_t *__restrict__ keys_out, uint64_t *__restrict__ vals_out,
                                                          uint32_t *__restrict__ flags) {
    __shared__ uint32_t wave_counts[kWaves][kDigits];
    __shared__ uint64_t digit_base[kDigits];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (the same trips for the whole workgroup)
        __syncthreads();
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) wave_counts[w][threadIdx.x] = 0u;
        __syncthreads();
        volatile uint32_t *mine = wave_counts[wave];
        const uint64_t first = t * kCanonicalUnitigSortTile + uint64_t(wave) * (kRounds * 64u) + lane;
        uint64_t key[kRounds], val[kRounds];
        uint32_t rank[kRounds];
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint64_t i = first + r * 64u;
            const bool live = i < n;
            key[r] = live ? keys_in[i] : 0ull;
            val[r] = live ? vals_in[i] : 0ull;
        }
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            const bool live = first + r * 64u < n;
            const uint32_t d = uint32_t(key[r] >> shift) & (kDigits - 1u);
            uint64_t peers = __ballot(live);  // the live lanes of the row with this lane's digit
#pragma unroll
            for (uint32_t b = 0; b < kDigitBits; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t with = __ballot(live && bit);
                peers &= bit ? with : ~with;
            }
            const uint32_t before = uint32_t(__popcll(peers & ((1ull << lane) - 1ull)));
            const uint32_t held = live ? mine[d] : 0u;
            __builtin_amdgcn_wave_barrier();
            if (live && before == 0u) mine[d] = held + uint32_t(__popcll(peers));
            __builtin_amdgcn_wave_barrier();
            rank[r] = held + before;
        }
        __syncthreads();
        {   // thread d: the digit's place in the output, and where each wave's share of it starts inside the tile's
            uint32_t acc = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t c = wave_counts[w][threadIdx.x];
                wave_counts[w][threadIdx.x] = acc;
                acc += c;
            }
            digit_base[threadIdx.x] = hist[uint64_t(threadIdx.x) * ntiles + t];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            if (first + r * 64u >= n) continue;
            const uint32_t d = uint32_t(key[r] >> shift) & (kDigits - 1u);
            const uint64_t to = digit_base[d] + wave_counts[wave][d] + rank[r];
            if (to >= n) {  // (the scanned histogram counts exactly n elements)
                atomicOr(flags, kFlagInternal);
                continue;
            }
            keys_out[to] = key[r];
            vals_out[to] = val[r];
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
            or_bits(edge_words, j, 1u << uint32_t(first_symbol));
            pred[j] = i;
            hairpins[0] += hairpin ? 1u : 0u;
        }
        if (out) or_bits(edge_words, i, out);
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
        clear_bits(g.link_words, i, kUnitigLinkUp);
        clear_bits(g.link_words, p, kUnitigLinkDown);
        state[i] = UnitigState{i, kUnitigDone};
        cut[0] += 1;
    }
    const uint64_t s = block_vector_sum(cut);
    if (threadIdx.x == 0 && s) {
        atomicAdd(counters + kCanonicalUnitigCut, (unsigned long long)s);
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
            or_bits(g.link_words, s.x, kUnitigSkip);
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

hipError_t canonical_unitig_sort(uint64_t *keys_a, uint64_t *vals_a, uint64_t *keys_b, uint64_t *vals_b, uint64_t N, uint32_t k, uint64_t *hist, uint64_t *scan,
                                 uint32_t *flags, hipStream_t stream, bool *in_b) {
    if (!keys_a || !vals_a || !keys_b || !vals_b || !hist || !scan || !flags || !in_b || k < 1 || k > 31) return hipErrorInvalidValue;
    *in_b = false;
    if (N < 2) return hipSuccess;
    const uint64_t ntiles = canonical_unitig_sort_tiles(N);
    if (scan_scratch_words(kDigits * ntiles) > canonical_unitig_scan_words(N)) return hipErrorInvalidValue;
    const dim3 grid(capped_grid(ntiles, 1, 1u << 16));
    const uint32_t passes = (2u * k + kDigitBits - 1u) / kDigitBits;  // the bytes above 2k bits are zero in every key
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t shift = pass * kDigitBits;
        hipLaunchKernelGGL(k_sort_histogram, grid, dim3(kThreads), 0, stream, keys_a, N, shift, ntiles, hist);
        const hipError_t e = exclusive_scan(hist, kDigits * ntiles, scan, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_sort_scatter, grid, dim3(kThreads), 0, stream, keys_a, vals_a, N, shift, ntiles, hist, keys_b, vals_b, flags);
        std::swap(keys_a, keys_b);
        std::swap(vals_a, vals_b);
        *in_b = !*in_b;
    }
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
