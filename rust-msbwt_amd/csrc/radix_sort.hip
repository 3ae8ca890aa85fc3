// gfx950 (MI355X, CDNA4): the stable 8-bit radix pass of radix_sort.hpp.  A workgroup of 256 threads takes a tile of 4096 pairs at a
// time (tile t = pairs [t * kRadixSortTile, ...)) and strides over the tiles; with the default grid cap that is one tile a workgroup up
// to 2^32 pairs.  Traffic per pair and pass: the key read for the histogram, key and payload read and written by the scatter.
// One writer per plain store: a tile's histogram column, and the place of a pair, which the scanned histogram gives to it alone.
// Integer only, no scratch memory (the arrays of a lane's kRounds pairs have constant indexes throughout).  No MFMA.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "kernels.hpp"
#include "radix_sort.hpp"
#include "run_encode.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr uint32_t kThreads = kScanThreads, kWaves = kScanWaves;
constexpr uint32_t kRounds = uint32_t(kRadixSortTile) / kThreads;  // pairs per lane in a tile
constexpr uint32_t kDigitBits = kRadixDigitBits, kDigits = 1u << kDigitBits;
static_assert(kRounds * kThreads == kRadixSortTile && kThreads == kDigits, "one thread per digit when a tile's counts are laid out");

// hist[digit * ntiles + tile] = the tile's elements with that digit
__global__ __launch_bounds__(256) void k_sort_histogram(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift, uint64_t ntiles, uint64_t *__restrict__ hist) {
    __shared__ uint32_t counts[kDigits];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (the same trips for the whole workgroup)
        counts[threadIdx.x] = 0u;
        __syncthreads();
        const uint64_t base = t * kRadixSortTile;
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
template <class Payload>
__global__ __launch_bounds__(256) void k_sort_scatter(const uint64_t *__restrict__ keys_in, const Payload *__restrict__ vals_in, uint64_t n, uint32_t shift, uint64_t ntiles,
                                                      const uint64_t *__restrict__ hist, uint64_t *__restrict__ keys_out, Payload *__restrict__ vals_out,
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
        const uint64_t first = t * kRadixSortTile + uint64_t(wave) * (kRounds * 64u) + lane;
        uint64_t key[kRounds];
        Payload val[kRounds];
        uint32_t rank[kRounds];
#pragma unroll
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint64_t i = first + r * 64u;
            const bool live = i < n;
            key[r] = live ? keys_in[i] : 0ull;
            val[r] = live ? vals_in[i] : Payload(0);
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
            asm volatile("" : "+v"(rank[r]));  // one register from here on: else the sum is sunk to the scatter below, and `peers` and `held` of all rows with it
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
                if (flags) atomicOr(flags, kFlagInternal);
                continue;
            }
            keys_out[to] = key[r];
            vals_out[to] = val[r];
        }
    }
}

// MSBWT_SORT_GRID=<workgroups>: (tests) lowers the cap on the passes' grids, so that a toy input meets the kernels' loops over tiles
uint32_t grid_cap() {
    constexpr uint32_t kDefault = 1u << 20;  // capped_grid's
    const char *e = std::getenv("MSBWT_SORT_GRID");
    const unsigned long long v = e ? std::strtoull(e, nullptr, 10) : 0ull;
    return v && v < kDefault ? uint32_t(v) : kDefault;
}

}  // namespace

template <class Payload>
hipError_t radix_sort_passes(uint64_t *keys_a, Payload *vals_a, uint64_t *keys_b, Payload *vals_b, uint64_t n, uint32_t shift0, uint32_t passes, uint64_t *hist,
                             uint64_t *scan, uint32_t *flags, hipStream_t stream, bool *in_b) {
    if (!keys_a || !vals_a || !keys_b || !vals_b || !hist || !scan || !in_b || shift0 + passes * kDigitBits > 64u) return hipErrorInvalidValue;
    *in_b = false;
    if (n < 2) return hipSuccess;
    const uint64_t ntiles = radix_sort_tiles(n);
    if (scan_scratch_words(kDigits * ntiles) > radix_sort_scan_words(n)) return hipErrorInvalidValue;
    const dim3 grid(capped_grid(ntiles, 1, grid_cap()));
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t shift = shift0 + pass * kDigitBits;
        hipLaunchKernelGGL(k_sort_histogram, grid, dim3(kThreads), 0, stream, keys_a, n, shift, ntiles, hist);
        const hipError_t e = exclusive_scan(hist, kDigits * ntiles, scan, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_sort_scatter<Payload>), grid, dim3(kThreads), 0, stream, keys_a, vals_a, n, shift, ntiles, hist, keys_b, vals_b, flags);
        std::swap(keys_a, keys_b);
        std::swap(vals_a, vals_b);
        *in_b = !*in_b;
    }
    return hipGetLastError();
}

template hipError_t radix_sort_passes<uint32_t>(uint64_t *, uint32_t *, uint64_t *, uint32_t *, uint64_t, uint32_t, uint32_t, uint64_t *, uint64_t *, uint32_t *, hipStream_t,
                                                bool *);
template hipError_t radix_sort_passes<uint64_t>(uint64_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t, uint32_t, uint32_t, uint64_t *, uint64_t *, uint32_t *, hipStream_t,
                                                bool *);

}  // namespace msbwt
