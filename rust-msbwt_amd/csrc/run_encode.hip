// The encoder of the device builders: a symbol array in HBM -> the RLE bytes of its runs, and the exclusive scan it and the
// builders' counting passes use.  Integer only, no scratch memory.
//
//   encode   run heads by comparison with the left neighbour, the next head by a suffix minimum, the bytes of a run (its
//            base-32 digit count) by a scan, then the digits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "run_encode.hpp"
#include "workgroup.hpp"

namespace msbwt {

namespace {

constexpr uint32_t kThreads = kScanThreads, kWaves = kScanWaves;
constexpr uint32_t kScanPer = 8, kScanChunk = kThreads * kScanPer;        // scan: elements per thread / workgroup
constexpr uint32_t kRunPer = 16, kRunTile = kThreads * kRunPer;            // encode: symbols per thread / workgroup
constexpr uint64_t kNone = ~0ull;

// minimum of v over the threads AFTER this one, `tail` beyond the last; *all = the minimum over every thread and tail.
// buf: 2 x kThreads words of LDS.
__device__ __forceinline__ uint64_t block_suffix_min(uint64_t v, uint64_t tail, uint64_t *buf, uint64_t *all) {
    const uint32_t t = threadIdx.x;
    uint32_t cur = 0;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        uint64_t x = buf[cur * kThreads + t];
        if (t + d < kThreads) x = min(x, buf[cur * kThreads + t + d]);
        buf[(cur ^ 1u) * kThreads + t] = x;
        __syncthreads();
        cur ^= 1u;
    }
    const uint64_t after = t + 1u < kThreads ? buf[cur * kThreads + t + 1u] : kNone;
    *all = min(buf[cur * kThreads], tail);
    return min(after, tail);
}

// ---- exclusive scan of u64, in place ----

__global__ __launch_bounds__(256) void k_scan_sums(const uint64_t *__restrict__ data, uint64_t n, uint64_t *__restrict__ sums) {
    __shared__ uint64_t wave_sums[kWaves];
    const uint64_t base = uint64_t(blockIdx.x) * kScanChunk + uint64_t(threadIdx.x) * kScanPer;
    uint64_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) s += base + i < n ? data[base + i] : 0ull;
    uint64_t total;
    block_exclusive_sum(s, wave_sums, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: the scanned workgroup sums, or nullptr for a single workgroup
__global__ __launch_bounds__(256) void k_scan_apply(uint64_t *__restrict__ data, uint64_t n, const uint64_t *__restrict__ sums) {
    __shared__ uint64_t wave_sums[kWaves];
    const uint64_t base = uint64_t(blockIdx.x) * kScanChunk + uint64_t(threadIdx.x) * kScanPer;
    uint64_t v[kScanPer], s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) {
        v[i] = base + i < n ? data[base + i] : 0ull;
        s += v[i];
    }
    uint64_t total;
    uint64_t acc = block_exclusive_sum(s, wave_sums, &total) + (sums ? sums[blockIdx.x] : 0ull);
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) {
        if (base + i < n) data[base + i] = acc;
        acc += v[i];
    }
}

}  // namespace

// words of scratch a scan of n elements needs (the sums of every level)
uint64_t scan_scratch_words(uint64_t n) {
    uint64_t words = 1;
    while (n > kScanChunk) {
        n = ceil_div(n, kScanChunk);
        words += n;
    }
    return words;
}

hipError_t exclusive_scan(uint64_t *d, uint64_t n, uint64_t *scratch, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = ceil_div(n, kScanChunk);
    if (blocks == 1) {
        hipLaunchKernelGGL(k_scan_apply, dim3(1), dim3(kThreads), 0, stream, d, n, static_cast<const uint64_t *>(nullptr));
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_scan_sums, dim3(uint32_t(blocks)), dim3(kThreads), 0, stream, d, n, scratch);
    hipError_t e = exclusive_scan(scratch, blocks, scratch + blocks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scan_apply, dim3(uint32_t(blocks)), dim3(kThreads), 0, stream, d, n, scratch);
    return hipGetLastError();
}

namespace {

// ---- step 5: symbols -> RLE bytes (src/msbwt_core.rs:3-14: symbol | digit << 3, base-32 digits, the lowest first) ----

// a thread's kRunPer consecutive symbols, and which of them start a run
struct RunSegment {
    uint64_t base;
    uint32_t live;          // symbols of the segment inside the array
    uint32_t heads;         // bit i: symbol i differs from its left neighbour (symbol 0 of the array is a head)
    uint8_t sym[kRunPer];
};

__device__ __forceinline__ RunSegment load_segment(const uint8_t *__restrict__ symbols, uint64_t n) {
    RunSegment s;
    s.base = uint64_t(blockIdx.x) * kRunTile + uint64_t(threadIdx.x) * kRunPer;
    s.live = s.base >= n ? 0u : uint32_t(min(uint64_t(kRunPer), n - s.base));
    s.heads = 0u;
    uint8_t left = s.base && s.live ? symbols[s.base - 1u] : uint8_t(0xFF);
#pragma unroll
    for (uint32_t i = 0; i < kRunPer; ++i) {
        s.sym[i] = i < s.live ? symbols[s.base + i] : uint8_t(0);
        if (i < s.live && s.sym[i] != left) s.heads |= 1u << i;
        left = s.sym[i];
    }
    return s;
}

__device__ __forceinline__ uint32_t digits_of(uint64_t len) { return (64u - uint32_t(__clzll((long long)len)) + 4u) / 5u; }

// first[tile] = the first run head inside the tile, kNone when it has none
__global__ __launch_bounds__(256) void k_run_first_heads(const uint8_t *__restrict__ symbols, uint64_t n, uint64_t *__restrict__ first) {
    __shared__ uint64_t buf[2 * kThreads];
    const RunSegment s = load_segment(symbols, n);
    const uint64_t mine = s.heads ? s.base + uint32_t(__ffs(s.heads) - 1) : kNone;
    uint64_t all;
    block_suffix_min(mine, kNone, buf, &all);
    if (threadIdx.x == 0) first[blockIdx.x] = all;
}

// first[t] <- the first run head in a tile after t, n when there is none.  One workgroup, from the last tile backwards.
__global__ __launch_bounds__(256) void k_run_next_heads(uint64_t *__restrict__ first, uint64_t ntiles, uint64_t n) {
    __shared__ uint64_t buf[2 * kThreads];
    uint64_t tail = n;
    for (uint64_t hi = ntiles; hi > 0; hi -= min(hi, uint64_t(kThreads))) {
        const uint64_t lo = hi > kThreads ? hi - kThreads : 0ull, t = lo + threadIdx.x;
        const uint64_t v = t < hi ? first[t] : kNone;
        uint64_t all;
        const uint64_t after = block_suffix_min(v, tail, buf, &all);
        if (t < hi) first[t] = after;
        tail = all;
    }
}

// the lengths of the runs that start in the thread's segment (0: not a head) and the bytes they take
__device__ __forceinline__ uint32_t run_lengths(const RunSegment &s, uint64_t next_head_after_tile, uint64_t *buf, uint64_t (&len)[kRunPer]) {
    const uint64_t mine = s.heads ? s.base + uint32_t(__ffs(s.heads) - 1) : kNone;
    uint64_t all;
    uint64_t next = block_suffix_min(mine, next_head_after_tile, buf, &all);
    uint32_t bytes = 0;
#pragma unroll
    for (uint32_t j = kRunPer; j-- > 0;) {
        len[j] = 0;
        if ((s.heads >> j) & 1u) {
            len[j] = next - (s.base + j);
            next = s.base + j;
            bytes += digits_of(len[j]);
        }
    }
    return bytes;
}

// bytes[tile] = RLE bytes of the runs that start in the tile; bytes[ntiles] = 0 (the scan leaves the total there)
__global__ __launch_bounds__(256) void k_run_bytes(const uint8_t *__restrict__ symbols, uint64_t n, const uint64_t *__restrict__ next_heads,
                                                   uint64_t *__restrict__ bytes) {
    __shared__ uint64_t buf[2 * kThreads];
    __shared__ uint64_t wave_sums[kWaves];
    const RunSegment s = load_segment(symbols, n);
    uint64_t len[kRunPer];
    const uint32_t mine = run_lengths(s, next_heads[blockIdx.x], buf, len);
    uint64_t total;
    block_exclusive_sum(uint64_t(mine), wave_sums, &total);
    if (threadIdx.x == 0) {
        bytes[blockIdx.x] = total;
        if (blockIdx.x + 1u == gridDim.x) bytes[gridDim.x] = 0ull;
    }
}

// bytes: scanned
__global__ __launch_bounds__(256) void k_run_write(const uint8_t *__restrict__ symbols, uint64_t n, const uint64_t *__restrict__ next_heads,
                                                   const uint64_t *__restrict__ bytes, uint8_t *__restrict__ rle) {
    __shared__ uint64_t buf[2 * kThreads];
    __shared__ uint64_t wave_sums[kWaves];
    const RunSegment s = load_segment(symbols, n);
    uint64_t len[kRunPer];
    const uint32_t mine = run_lengths(s, next_heads[blockIdx.x], buf, len);
    uint64_t total;
    uint64_t at = bytes[blockIdx.x] + block_exclusive_sum(uint64_t(mine), wave_sums, &total);  // + the run's digits <= bytes[ntiles], the buffer's size
#pragma unroll
    for (uint32_t j = 0; j < kRunPer; ++j)
        for (uint64_t left = len[j]; left > 0; left >>= 5) rle[at++] = uint8_t(s.sym[j] | ((left & 31u) << 3));
}

}  // namespace

hipError_t encode_symbol_runs(Arena &arena, const uint8_t *d_symbols, uint64_t total, hipStream_t stream, uint8_t **d_rle_out, uint64_t *rle_bytes,
                              const char **what) {
    hipError_t e = hipSuccess;
    auto failed = [&](const char *step) {
        *what = step;
        return e;
    };
    const uint64_t run_tiles = ceil_div(total, kRunTile);
    uint64_t *d_heads = nullptr, *d_bytes = nullptr, need = 0;
    uint8_t *d_rle = nullptr;
    if ((e = arena.take(&d_heads, run_tiles * 8)) != hipSuccess || (e = arena.take(&d_bytes, (run_tiles + 1 + scan_scratch_words(run_tiles + 1)) * 8)) != hipSuccess)
        return failed("the buffers of the encoder");
    hipLaunchKernelGGL(k_run_first_heads, dim3(uint32_t(run_tiles)), dim3(kThreads), 0, stream, d_symbols, total, d_heads);
    hipLaunchKernelGGL(k_run_next_heads, dim3(1), dim3(kThreads), 0, stream, d_heads, run_tiles, total);
    hipLaunchKernelGGL(k_run_bytes, dim3(uint32_t(run_tiles)), dim3(kThreads), 0, stream, d_symbols, total, d_heads, d_bytes);
    if ((e = exclusive_scan(d_bytes, run_tiles + 1, d_bytes + run_tiles + 1, stream)) != hipSuccess) return failed("sizing the runs");
    if ((e = hipMemcpyAsync(&need, d_bytes + run_tiles, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess || (e = hipStreamSynchronize(stream)) != hipSuccess)
        return failed("sizing the runs");
    if (need == 0 || need > total) {
        *what = "the run lengths do not add up (a bug)";
        return hipErrorUnknown;
    }
    if ((e = arena.take(&d_rle, need)) != hipSuccess) return failed("the RLE bytes in HBM");
    hipLaunchKernelGGL(k_run_write, dim3(uint32_t(run_tiles)), dim3(kThreads), 0, stream, d_symbols, total, d_heads, d_bytes, d_rle);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(stream)) != hipSuccess) return failed("writing the runs");
    arena.give_back(d_heads);
    arena.give_back(d_bytes);
    *d_rle_out = d_rle;
    *rle_bytes = need;
    return hipSuccess;
}

}  // namespace msbwt
