// The wave and workgroup primitives of the device builders (loader, merges, encoder, builder from reads) and of the frontier
// walks: launch arithmetic, wave sums and maxima, the workgroup prefix sum, the workgroup sum of a small vector (and its addition
// to counters in HBM), and the one-workgroup scan of per-tile vectors.  Include from HIP translation units only (the names are per translation unit, as in frontier.hpp).
// Integer only, and no instantiation needs scratch memory: every loop over waves or elements has a constant bound.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace msbwt {
namespace {

__host__ __device__ inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// workgroups for `items` at `per_block` each: at least one, at most `cap` (the kernels stride over what is left)
inline uint32_t capped_grid(uint64_t items, uint64_t per_block, uint32_t cap = 1u << 20) {
    return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(cap, ceil_div(items, per_block))));
}

// sum of v over this lane and the lanes of the wave below it (T: uint32_t or uint64_t).  The whole wave calls it.
template <class T>
__device__ __forceinline__ T wave_inclusive_sum(T v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// sum of v over the wave, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the largest v of the wave, in every lane
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const T other = __shfl_xor(v, d);
        v = other > v ? other : v;
    }
    return v;
}

// exclusive prefix sum of v over the workgroup's kWaves x 64 threads; *total = the sum.  wave_sums: kWaves words of LDS, free
// again at the next call's first barrier.  The builders run 256 threads: kWaves = 4.
template <uint32_t kWaves = 4, class T>
__device__ __forceinline__ T block_exclusive_sum(T v, T *wave_sums, T *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_sum(v);
    __syncthreads();  // the words are free again
    if (lane == 63u) wave_sums[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        const T s = wave_sums[w];
        before += w < wave ? s : T(0);
        all += s;
    }
    *total = all;
    return before + incl - v;
}

// the workgroup's sums of v[0 .. N): thread k < N returns the sum of v[k] (the others return 0).  Every thread of the workgroup
// calls it (it opens with a barrier), and every instantiation has N x kWaves words of LDS of its own.
template <uint32_t kWaves = 4, class T, uint32_t N>
__device__ __forceinline__ uint64_t block_vector_sum(const T (&v)[N]) {
    __shared__ T part[N][kWaves];
    __syncthreads();  // the words are free again
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
        const T x = wave_sum(v[k]);
        if ((threadIdx.x & 63u) == 0u) part[k][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    uint64_t s = 0;
    if (threadIdx.x < N) {
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) s += part[threadIdx.x][w];
    }
    return s;
}

// counters[at + j] += the workgroup's sum of v[j], which thread j < N returns as block_vector_sum does; the whole workgroup calls it
template <uint32_t N>
__device__ __forceinline__ uint64_t add_to_counters(unsigned long long *__restrict__ counters, uint32_t at, const uint64_t (&v)[N]) {
    const uint64_t s = block_vector_sum(v);
    if (threadIdx.x < N && s) atomicAdd(counters + at + threadIdx.x, (unsigned long long)s);
    return s;
}

// N sums per tile of a builder's input, and their scan over the tiles
template <uint32_t N>
struct TileSums {
    uint64_t v[N];
};

// In-place exclusive scan of tiles[0 .. ntiles) element by element; totals (N words, or nullptr) gets the grand totals.  One
// workgroup of 1024 threads: rounds of 1024 tiles (a tile's N sums are read together), the sums so far carried in LDS.
template <uint32_t N>
__global__ __launch_bounds__(1024) void k_scan_tile_sums(TileSums<N> *__restrict__ tiles, uint64_t ntiles, uint64_t *__restrict__ totals) {
    static_assert(N >= 2, "carry[k] is written behind the barriers of element k and read before them a round later: another element's lie between");
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t carry[N];
    if (threadIdx.x < N) carry[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t base = 0; base < ntiles; base += 1024) {
        const uint64_t t = base + threadIdx.x;
#pragma unroll 1
        for (uint32_t k = 0; k < N; ++k) {
            const uint64_t x = t < ntiles ? tiles[t].v[k] : 0, so_far = carry[k];
            uint64_t all;
            const uint64_t before = block_exclusive_sum<16>(x, wave_sums, &all);
            if (t < ntiles) tiles[t].v[k] = so_far + before;
            if (threadIdx.x == 0) carry[k] = so_far + all;
        }
    }
    __syncthreads();
    if (totals && threadIdx.x < N) totals[threadIdx.x] = carry[threadIdx.x];
}

}  // namespace
}  // namespace msbwt
