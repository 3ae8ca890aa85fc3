// Device-side index build (load path): RLE bytes in HBM -> plane blocks, without ever holding
// the expanded index on the host.  Three kernels and a small scan:
//
//   k_tile_sums   every 4 KiB tile of RLE bytes -> {symbols, per-symbol counts} it encodes
//   k_scan_tile_sums<7>  exclusive prefix over the tiles (7 x u64 per tile; workgroup.hpp, shared with pair_index.hip)
//   k_paint       every byte is one "sub-run" (digit << 5*index-in-its-run symbols of one
//                 code): a block-level scan gives its BWT position and the symbol counts
//                 before it; the thread ORs its bits into the planes (atomicOr: neighbouring
//                 sub-runs share words) and writes the header of every block whose first
//                 position it covers.  Sub-runs of >= 2048 symbols go to a list ...
//   k_paint_long  ... and are filled by one workgroup each with plain stores.
//
// This is what breaks the carry chain of the on-disk format (the weight of a byte depends on
// how many bytes of the same symbol precede it, reference src/rle_bwt.rs:360-371): the
// exponent is found by looking back at most 16 bytes, everything else is a prefix sum.  The walk over a thread's bytes is
// rle_subruns.hpp's (shared with the merge decoder), the sums and scans inside a workgroup are workgroup.hpp's.
#include <hip/hip_runtime.h>

#include "device_build.hpp"
#include "plane_index.hpp"
#include "rle_subruns.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = 256;
constexpr int kBytesPerThread = 16;
constexpr int kTileBytes = kThreads * kBytesPerThread;  // 4096
constexpr uint64_t kLongRun = 2048;                      // symbols; longer sub-runs are deferred

using Seven = TileSums<7>;  // [0..5] per-symbol counts, [6] all symbols

struct LongRun {
    uint64_t pos, len;
    uint64_t occ[6];  // symbol counts before pos
    uint32_t sym, pad;
};

// acc[sym] += v without a runtime-indexed register array
__device__ __forceinline__ void add_to_symbol(uint64_t acc[7], uint32_t sym, uint64_t v) {
#pragma unroll
    for (int s = 0; s < 6; ++s) acc[s] += (uint32_t(s) == sym) ? v : 0;
}

__global__ __launch_bounds__(kThreads) void k_tile_sums(const uint8_t *__restrict__ rle, uint64_t n,
                                                        Seven *__restrict__ tile_sums, uint32_t *__restrict__ flags,
                                                        unsigned long long *__restrict__ long_count) {
    for (uint64_t tile = blockIdx.x; tile * kTileBytes < n; tile += gridDim.x) {
        const uint64_t first = tile * kTileBytes + uint64_t(threadIdx.x) * kBytesPerThread;
        const ThreadBytes tb = load_thread_bytes(rle, n, first);
        uint64_t acc[7] = {0, 0, 0, 0, 0, 0, 0};
        uint32_t longs = 0;
        const uint32_t bad = for_each_subrun(tb, [&](uint32_t sym, uint64_t v) {
            add_to_symbol(acc, sym, v);
            acc[6] += v;
            longs += (v >= kLongRun) ? 1u : 0u;
        });
        if (bad) atomicOr(flags, bad);
        if (longs) atomicAdd(long_count, (unsigned long long)longs);
        const uint64_t sum = block_vector_sum(acc);
        if (threadIdx.x < 7) tile_sums[tile].v[threadIdx.x] = sum;
    }
}

// Header words of block `b` from the bounds A[s] (layout: plane_index.hpp)
__device__ __forceinline__ void store_meta(uint32_t *__restrict__ blocks, uint64_t b, const uint64_t A[6]) {
    uint32_t *blk = blocks + b * 32;
    uint32_t hi_a = 0, hi_b = 0;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        blk[4 * s + 3] = uint32_t(A[s]);
        const uint32_t hi = uint32_t(A[s] >> 32) & 0xFFu;
        if (s < 4) hi_a |= hi << (8 * s);
        else hi_b |= hi << (8 * (s - 4));
    }
    blk[4 * 6 + 3] = hi_a;
    blk[4 * 7 + 3] = hi_b;
}

// OR symbol `sym` into positions [pos, pos+len) of the planes, word by word.
__device__ __forceinline__ void paint_atomic(uint32_t *__restrict__ blocks, uint32_t sym, uint64_t pos, uint64_t len) {
    const uint64_t end = pos + len;
    for (uint64_t w = pos >> 5; w <= (end - 1) >> 5; ++w) {
        const uint32_t lo = uint32_t(max(pos, w << 5) - (w << 5));
        const uint32_t hi = uint32_t(min(end, (w << 5) + 32) - (w << 5));  // 1..32
        const uint32_t mask = (hi == 32u ? ~0u : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
        uint32_t *word = blocks + (w >> 3) * 32 + (w & 7u) * 4;
        if (sym & 1u) atomicOr(word + 0, mask);
        if (sym & 2u) atomicOr(word + 1, mask);
        if (sym & 4u) atomicOr(word + 2, mask);
    }
}

// Headers of every block whose first position lies in [pos, pos+len): occ[] = counts before pos.
__device__ __forceinline__ void write_headers(uint32_t *__restrict__ blocks, const uint64_t *__restrict__ start_index,
                                              uint32_t sym, uint64_t pos, uint64_t len, const uint64_t occ[6]) {
    for (uint64_t B = (pos + 255) & ~uint64_t(255); B < pos + len; B += 256) {
        uint64_t A[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) A[s] = start_index[s] + occ[s] + (uint32_t(s) == sym ? B - pos : 0);
        store_meta(blocks, B >> 8, A);
    }
}

__global__ __launch_bounds__(kThreads) void k_paint(const uint8_t *__restrict__ rle, uint64_t n,
                                                    const Seven *__restrict__ tile_base,
                                                    const uint64_t *__restrict__ start_index,
                                                    uint32_t *__restrict__ blocks, LongRun *__restrict__ long_runs,
                                                    unsigned long long *__restrict__ long_cursor) {
    __shared__ uint64_t lds4[kThreads / 64];
    for (uint64_t tile = blockIdx.x; tile * kTileBytes < n; tile += gridDim.x) {
        const uint64_t first = tile * kTileBytes + uint64_t(threadIdx.x) * kBytesPerThread;
        const ThreadBytes tb = load_thread_bytes(rle, n, first);
        uint64_t mine[7] = {0, 0, 0, 0, 0, 0, 0};
        (void)for_each_subrun(tb, [&](uint32_t sym, uint64_t v) {
            add_to_symbol(mine, sym, v);
            mine[6] += v;
        });
        // position and per-symbol counts at this thread's first byte
        uint64_t at[7], dummy;
        for (int k = 0; k < 7; ++k) at[k] = tile_base[tile].v[k] + block_exclusive_sum(mine[k], lds4, &dummy);
        (void)for_each_subrun(tb, [&](uint32_t sym, uint64_t v) {
            if (v == 0) return;
            const uint64_t pos = at[6];
            if (v >= kLongRun) {
                const unsigned long long slot = atomicAdd(long_cursor, 1ull);
                LongRun lr;
                lr.pos = pos;
                lr.len = v;
                for (int s = 0; s < 6; ++s) lr.occ[s] = at[s];
                lr.sym = sym;
                lr.pad = 0;
                long_runs[slot] = lr;
            } else {
                if (sym) paint_atomic(blocks, sym, pos, v);
                write_headers(blocks, start_index, sym, pos, v, at);
            }
            add_to_symbol(at, sym, v);
            at[6] += v;
        });
    }
}

// One workgroup per long sub-run: partial words at both ends by atomicOr, whole words in
// between by plain stores (nothing else writes them), headers for every covered block.
__global__ __launch_bounds__(kThreads) void k_paint_long(const LongRun *__restrict__ long_runs, uint64_t nlong,
                                                         const uint64_t *__restrict__ start_index,
                                                         uint32_t *__restrict__ blocks) {
    for (uint64_t item = blockIdx.x; item < nlong; item += gridDim.x) {
        const LongRun lr = long_runs[item];
        const uint64_t pos = lr.pos, end = lr.pos + lr.len;
        const uint64_t first_full = (pos + 31) >> 5, last_full = end >> 5;  // words [first_full, last_full) are whole
        if (lr.sym) {
            if (threadIdx.x == 0 && (pos & 31u)) paint_atomic(blocks, lr.sym, pos, min(end, first_full << 5) - pos);
            if (threadIdx.x == 1 && (end & 31u) && (last_full >= first_full)) paint_atomic(blocks, lr.sym, last_full << 5, end - (last_full << 5));
            for (uint64_t w = first_full + threadIdx.x; w < last_full; w += kThreads) {
                uint32_t *word = blocks + (w >> 3) * 32 + (w & 7u) * 4;
                if (lr.sym & 1u) word[0] = ~0u;
                if (lr.sym & 2u) word[1] = ~0u;
                if (lr.sym & 4u) word[2] = ~0u;
            }
        }
        const uint64_t B0 = (pos + 255) & ~uint64_t(255);
        for (uint64_t B = B0 + uint64_t(threadIdx.x) * 256; B < end; B += uint64_t(kThreads) * 256) {
            uint64_t A[6];
#pragma unroll
            for (int s = 0; s < 6; ++s) A[s] = start_index[s] + lr.occ[s] + (uint32_t(s) == lr.sym ? B - pos : 0);
            store_meta(blocks, B >> 8, A);
        }
    }
}

// Header of the block that starts exactly at T (no sub-run covers that position).
__global__ void k_final_header(const uint64_t *__restrict__ start_index, const uint64_t *__restrict__ totals,
                               uint32_t *__restrict__ blocks) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && (totals[6] & 255u) == 0) {
        uint64_t A[6];
        for (int s = 0; s < 6; ++s) A[s] = start_index[s] + totals[s];
        store_meta(blocks, totals[6] >> 8, A);
    }
}

}  // namespace

size_t device_build_scratch_bytes(size_t n) {
    const uint64_t ntiles = ceil_div(n, kTileBytes);
    return size_t(ntiles + 1) * sizeof(Seven) + 256;
}

hipError_t device_build_pass1(const uint8_t *d_rle, size_t n, void *d_scratch, DeviceBuildState *st, hipStream_t stream) {
    // scratch: [totals 7 x u64 | start_index 6 x u64 | flags u32 | long_count u64 | long_cursor u64] + tile sums
    uint8_t *base = static_cast<uint8_t *>(d_scratch);
    st->d_totals = reinterpret_cast<uint64_t *>(base);
    st->d_start_index = st->d_totals + 7;
    st->d_flags = reinterpret_cast<uint32_t *>(st->d_start_index + 6);
    st->d_long_count = reinterpret_cast<unsigned long long *>(st->d_start_index + 8);
    st->d_long_cursor = st->d_long_count + 1;
    st->d_tiles = base + 256;
    st->ntiles = ceil_div(n, kTileBytes);
    hipError_t e = hipMemsetAsync(base, 0, 256, stream);
    if (e != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tile_sums, dim3(capped_grid(st->ntiles, 1, 4096)), dim3(kThreads), 0, stream, d_rle, uint64_t(n),
                       static_cast<Seven *>(st->d_tiles), st->d_flags, st->d_long_count);
    hipLaunchKernelGGL(k_scan_tile_sums<7>, dim3(1), dim3(1024), 0, stream, static_cast<Seven *>(st->d_tiles), st->ntiles, st->d_totals);
    return hipGetLastError();
}

hipError_t device_build_pass2(const uint8_t *d_rle, size_t n, const DeviceBuildState &st, void *d_long_runs,
                              uint64_t nlong, void *d_blocks, hipStream_t stream) {
    uint32_t *blocks = static_cast<uint32_t *>(d_blocks);
    if (n) {
        hipLaunchKernelGGL(k_paint, dim3(capped_grid(st.ntiles, 1, 4096)), dim3(kThreads), 0, stream, d_rle, uint64_t(n),
                           static_cast<const Seven *>(st.d_tiles), st.d_start_index, blocks,
                           static_cast<LongRun *>(d_long_runs), st.d_long_cursor);
        if (nlong)
            hipLaunchKernelGGL(k_paint_long, dim3(capped_grid(nlong, 1, 2048)), dim3(kThreads), 0, stream,
                               static_cast<const LongRun *>(d_long_runs), nlong, st.d_start_index, blocks);
    }
    hipLaunchKernelGGL(k_final_header, dim3(1), dim3(64), 0, stream, st.d_start_index, st.d_totals, blocks);
    return hipGetLastError();
}

size_t device_build_long_run_bytes(uint64_t nlong) { return size_t(nlong ? nlong : 1) * sizeof(LongRun); }

}  // namespace msbwt
