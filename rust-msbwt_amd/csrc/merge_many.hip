// Merge of any number of inputs in one pass: the BWTs of up to kMergeMaxInputs read sets -> the BWT of their union and, for every
// merged row, the input it came from.  The iteration of merge.hip (Holt & McMillan 2014) with a byte per merged row, the input's
// index, in place of a bit.
//
// The array starts as the rows of input 0, then input 1, and so on.  One iteration reads the rows' symbols in the order the
// array gives and sends every row's byte to (rows with a smaller symbol) + (rows with the same symbol before it): a stable
// six-way counting sort of the array by symbol.  When an iteration changes nothing the array is the interleave of the union's
// BWT; rows of equal rotations stay in input order, because the sort is stable and they started so.
//
//   1. decode    merge.hip's decoder, input by input, into one symbol array (every input at a 16-byte border).
//   2. iterate   tiles of kMergeTile rows.  a) the tile's rows per input, input-major, one scan over inputs x tiles: the scanned
//                count is where the tile's slice of that input starts among all decoded symbols (inside a tile the rows of one
//                input are a contiguous slice of it: the loads coalesce).  b) the tile's six symbol counts (of the slices as
//                they lie), symbol-major, one scan over 6 x tiles: the scanned counts are the rows' destinations.  c) the
//                slices staged in LDS; a row's symbol is at its rank among the tile's rows of the same input, from workgroup
//                scans over 16-bit counts, four inputs to a word, words of absent inputs skipped; per symbol the rows' bytes
//                are strung together in LDS at the alignment of their place in the next array and written there, single bytes
//                up to the first 16-byte border and after the last, 16-byte stores between.  Every row is written exactly
//                once: no memset, no atomics.  What is written is compared with the current array on the way: one word back
//                to the host.
//   3. emit      the merged symbols, through the final array.
//   4. encode    run_encode.hip, as the builder from reads.
//
// Integer only; every kernel runs without scratch memory.  Every row index and offset is 64-bit; 32-bit are counts and ranks
// inside one tile (<= kMergeTile).
#include "merge_common.hpp"

namespace msbwt {

namespace {

constexpr uint32_t kGroups = kMergeMaxInputs / 4;     // words of four 16-bit counts, one count per input
constexpr uint32_t kStrung = kMergeTile + kSymbols * 32;  // the six strings: each starts at most 15 bytes into a 16-byte line of its own
static_assert(kRowsPer == 16 && kMergeMaxInputs == 32 && kMergeTile <= 0xFFFFu, "a thread holds 16 bytes of the array; a count of a tile fits 16 bits");

struct ManyInputs {
    const uint8_t *sym;     // the decoded inputs, one after the other
    const uint64_t *shift;  // [n] bytes of padding in `sym` before input i's first symbol, in all
    uint64_t sym_bytes;     // bytes of `sym`
    uint64_t total;         // merged rows
    uint32_t n;
};

// a thread's kRowsPer consecutive bytes of the array
struct Bytes {
    uint32_t w[4];
    __device__ __forceinline__ uint32_t at(uint32_t j) const { return (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu; }
};

__device__ __forceinline__ Bytes load_bytes(const uint8_t *__restrict__ src, uint64_t at) {  // (the arrays hold whole tiles)
    const uint4 v = *reinterpret_cast<const uint4 *>(src + at);
    return Bytes{{v.x, v.y, v.z, v.w}};
}

// how many of a thread's rows are inside the array
__device__ __forceinline__ uint32_t live_rows(uint64_t total) {
    const uint64_t base = uint64_t(blockIdx.x) * kMergeTile + uint64_t(threadIdx.x) * kRowsPer;
    return base >= total ? 0u : uint32_t(min(uint64_t(kRowsPer), total - base));
}

// the thread's rows of inputs 4 g .. 4 g + 3, 16 bits each
__device__ __forceinline__ uint64_t count_group(const Bytes &b, uint32_t live, uint32_t g) {
    uint64_t w = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) {
        const uint32_t d = b.at(j) - 4u * g;
        w += j < live && d < 4u ? 1ull << (16u * d) : 0ull;
    }
    return w;
}

// ---- 2 a. rows per tile and input ----

// counts[input * ntiles + tile] = the tile's rows of that input
__global__ __launch_bounds__(256) void k_many_input_counts(const uint8_t *__restrict__ src, uint64_t total, uint32_t n, uint64_t ntiles, uint64_t *__restrict__ counts) {
    __shared__ uint64_t wave_sums[kScanWaves];
    __shared__ uint32_t wave_seen[kScanWaves];
    const uint32_t t = threadIdx.x, live = live_rows(total);
    const Bytes b = load_bytes(src, uint64_t(blockIdx.x) * kMergeTile + uint64_t(t) * kRowsPer);
    uint32_t seen = 0;  // bit i: a row of input i
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) seen |= j < live ? 1u << (b.at(j) & 31u) : 0u;
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) seen |= __shfl_xor(seen, d);
    if ((t & 63u) == 0u) wave_seen[t >> 6] = seen;
    __syncthreads();
    seen = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScanWaves; ++w) seen |= wave_seen[w];
#pragma unroll 1
    for (uint32_t g = 0; 4u * g < n; ++g) {
        uint64_t all = 0;
        if ((seen >> (4u * g)) & 0xFu) block_exclusive_sum(count_group(b, live, g), wave_sums, &all);  // (the same branch in every thread)
        if (t < 4u && 4u * g + t < n) counts[uint64_t(4u * g + t) * ntiles + blockIdx.x] = (all >> (16u * t)) & 0xFFFFu;
    }
}

// ---- the tile's slices ----

struct TileMap {
    uint32_t pre[kMergeMaxInputs];   // rows of the tile's slices before input i's; ~0 from input n on
    uint64_t from[kMergeMaxInputs];  // where input i's slice starts in `sym`, minus pre[i]
    uint32_t present;                // bit i: the tile holds rows of input i
};

// starts: the scanned counts.  Wave 0 calls it; a barrier publishes the map.
__device__ __forceinline__ void make_map(TileMap &map, const uint64_t *__restrict__ starts, const ManyInputs &in, uint64_t ntiles) {
    const uint32_t i = threadIdx.x;
    uint64_t start = 0;
    uint32_t c = 0;
    if (i < in.n) {
        const uint64_t at = uint64_t(i) * ntiles + blockIdx.x, end = at + 1u < uint64_t(in.n) * ntiles ? starts[at + 1u] : in.total;
        start = starts[at];
        c = uint32_t(min(end - start, uint64_t(kMergeTile)));
    }
    const uint32_t incl = wave_inclusive_sum(c);
    const unsigned long long has = __ballot(c > 0u);
    if (i < kMergeMaxInputs) {
        map.pre[i] = i < in.n ? incl - c : ~0u;
        map.from[i] = i < in.n ? start + in.shift[i] - (incl - c) : 0ull;
    }
    if (i == 0u) map.present = uint32_t(has);
}

// symbol k of the tile's rows taken input by input.  The load itself is unconditional (of the array's last byte when the index
// is past it, which it is not while the array holds every input's rows), so that a thread's loads are all in flight at once.
__device__ __forceinline__ uint32_t slice_symbol(const TileMap &map, const ManyInputs &in, uint32_t k) {
    uint32_t i = 0;
#pragma unroll
    for (uint32_t step = kMergeMaxInputs / 2; step > 0; step >>= 1) i += map.pre[i + step] <= k ? step : 0u;  // the last slice that starts at or before k
    return in.sym[min(map.from[i] + k, in.sym_bytes - 1u)];
}

// ---- 2 b. symbols per tile ----

// hist[symbol * ntiles + tile] = the tile's rows with that symbol.  The counts do not depend on the order of the rows inside
// the tile, so the slices are counted as they lie.
__global__ __launch_bounds__(256) void k_many_histogram(const uint64_t *__restrict__ starts, ManyInputs in, uint64_t ntiles, uint64_t *__restrict__ hist) {
    __shared__ TileMap map;
    __shared__ uint64_t wave_sums[kScanWaves];
    if (threadIdx.x < 64u) make_map(map, starts, in, ntiles);
    __syncthreads();
    const uint32_t valid = uint32_t(min(uint64_t(kMergeTile), in.total - uint64_t(blockIdx.x) * kMergeTile));
    uint64_t a = 0, b = 0, all_a, all_b;
#pragma unroll
    for (uint32_t r = 0; r < kRowsPer; ++r) {
        const uint32_t k = r * kThreads + threadIdx.x, s = slice_symbol(map, in, k);
        count_symbol(k < valid ? s : kNoRow, &a, &b);
    }
    block_exclusive_sum(a, wave_sums, &all_a);
    block_exclusive_sum(b, wave_sums, &all_b);
    if (threadIdx.x < kSymbols) hist[uint64_t(threadIdx.x) * ntiles + blockIdx.x] = field(all_a, all_b, threadIdx.x);
}

// ---- 2 c. the rows of a tile, their symbols, the scatter ----

struct TileShared {
    TileMap map;
    uint64_t wave_sums[kScanWaves];
    uint8_t stage[kMergeTile];  // the tile's symbols, slice by slice
};

struct Rows {
    Bytes from;     // the inputs of the thread's rows
    uint64_t syms;  // their symbols, 3 bits each, kNoRow past the last row
};

// Every thread of the workgroup calls it, once.
__device__ __forceinline__ Rows load_rows(TileShared &sh, const uint8_t *__restrict__ src, const uint64_t *__restrict__ starts, const ManyInputs &in, uint64_t ntiles) {
    const uint32_t t = threadIdx.x, live = live_rows(in.total);
    if (t < 64u) make_map(sh.map, starts, in, ntiles);
    Rows r;
    r.from = load_bytes(src, uint64_t(blockIdx.x) * kMergeTile + uint64_t(t) * kRowsPer);
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kRowsPer; ++q) sh.stage[q * kThreads + t] = uint8_t(slice_symbol(sh.map, in, q * kThreads + t));  // (past the tile's last row: not read)
    __syncthreads();
    const uint32_t present = sh.map.present;
    r.syms = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) r.syms |= j < live ? 0ull : uint64_t(kNoRow) << (3u * j);
#pragma unroll 1
    for (uint32_t g = 0; g < kGroups; ++g) {
        if (!((present >> (4u * g)) & 0xFu)) continue;  // (the same branch in every thread)
        uint64_t all;
        uint64_t rank = block_exclusive_sum(count_group(r.from, live, g), sh.wave_sums, &all);  // of the thread's next row of each of the four inputs
#pragma unroll
        for (uint32_t j = 0; j < kRowsPer; ++j) {
            const uint32_t i = r.from.at(j), d = i - 4u * g;
            if (j < live && d < 4u) {
                const uint32_t at = (sh.map.pre[i & (kMergeMaxInputs - 1u)] + uint32_t((rank >> (16u * d)) & 0xFFFFu)) & (kMergeTile - 1u);
                rank += 1ull << (16u * d);
                r.syms |= uint64_t(sh.stage[at] & 7u) << (3u * j);
            }
        }
    }
    return r;
}

// hist: scanned.  Every row of `next` below in.total is written, once.  *flag: set when a byte written differs from cur's.
__global__ __launch_bounds__(256) void k_many_scatter(const uint8_t *__restrict__ cur, const uint64_t *__restrict__ starts, ManyInputs in, uint64_t ntiles,
                                                      const uint64_t *__restrict__ hist, uint8_t *__restrict__ next, uint32_t *__restrict__ flag) {
    __shared__ TileShared sh;
    __shared__ __attribute__((aligned(16))) uint8_t strung[kStrung];
    __shared__ uint64_t offsets[kSymbols];
    __shared__ uint32_t begins[kSymbols];
    const uint32_t t = threadIdx.x;
    if (t < kSymbols) offsets[t] = hist[uint64_t(t) * ntiles + blockIdx.x];
    const Rows r = load_rows(sh, cur, starts, in, ntiles);  // (its barriers publish the offsets)
    uint64_t a = 0, b = 0, all_a, all_b;
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) count_symbol(uint32_t(r.syms >> (3u * j)) & 7u, &a, &b);
    uint64_t rank_a = block_exclusive_sum(a, sh.wave_sums, &all_a), rank_b = block_exclusive_sum(b, sh.wave_sums, &all_b);
    if (t == 0u) {  // a string begins where its rows' place in `next` begins within a 16-byte line
        uint32_t line = 0;
#pragma unroll
        for (uint32_t s = 0; s < kSymbols; ++s) {
            begins[s] = line + uint32_t(offsets[s] & 15u);
            line = (begins[s] + field(all_a, all_b, s) + 15u) & ~15u;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) {
        const uint32_t s = uint32_t(r.syms >> (3u * j)) & 7u;
        if (s < kSymbols) {
            strung[min(begins[s] + field(rank_a, rank_b, s), kStrung - 1u)] = uint8_t(r.from.at(j));
            count_symbol(s, &rank_a, &rank_b);
        }
    }
    __syncthreads();
    bool differs = false;
#pragma unroll
    for (uint32_t s = 0; s < kSymbols; ++s) {
        const uint32_t count = field(all_a, all_b, s);
        if (count == 0u) continue;
        const uint64_t hi = min(in.total, offsets[s] + count), lo = min(hi, offsets[s]);  // (the scanned counts end at the last row)
        const uint64_t body_lo = min(hi, (lo + 15u) & ~15ull), body_hi = max(body_lo, hi & ~15ull);
        const uint8_t *string = strung + begins[s];  // string[x - lo]: the byte of row x
        if (lo + t < body_lo) {
            const uint8_t v = string[t];
            differs = differs || cur[lo + t] != v;
            next[lo + t] = v;
        }
        const uint64_t x = body_lo + uint64_t(t) * 16u;  // (a string has at most kMergeTile bytes: one round)
        if (x < body_hi) {
            const uint4 v = *reinterpret_cast<const uint4 *>(string + (x - lo)), was = *reinterpret_cast<const uint4 *>(cur + x);
            differs = differs || v.x != was.x || v.y != was.y || v.z != was.z || v.w != was.w;
            *reinterpret_cast<uint4 *>(next + x) = v;
        }
        if (body_hi + t < hi) {
            const uint8_t v = string[body_hi + t - lo];
            differs = differs || cur[body_hi + t] != v;
            next[body_hi + t] = v;
        }
    }
    if (differs) *flag = 1u;
}

// ---- 3. emit ----

// merged: whole tiles
__global__ __launch_bounds__(256) void k_many_emit(const uint8_t *__restrict__ src, const uint64_t *__restrict__ starts, ManyInputs in, uint64_t ntiles,
                                                   uint8_t *__restrict__ merged) {
    __shared__ TileShared sh;
    const Rows r = load_rows(sh, src, starts, in, ntiles);
    *reinterpret_cast<uint4 *>(merged + uint64_t(blockIdx.x) * kMergeTile + uint64_t(threadIdx.x) * kRowsPer) = merged_symbols(r.syms);
}

// ---- the byte state under run_merge ----

struct ByteState {
    using Word = uint8_t;
    static uint64_t plan(const MergeJob &job) { return plan_merge_many(job.total); }
    static uint64_t state_bytes(const MergeJob &job) { return job.ntiles * kMergeTile; }  // whole tiles: a thread loads 16 bytes
    static uint64_t out_bytes(const MergeJob &job) { return job.total; }
    static uint64_t counts(const MergeJob &job) { return job.n; }  // the tile's rows of every input

    const MergeJob &job;
    const uint32_t tile_grid;
    ManyInputs inputs;
    explicit ByteState(const MergeJob &j) : job(j), tile_grid(uint32_t(j.ntiles)), inputs{j.d_sym, nullptr, j.sym_bytes, j.total, j.n} {}

    hipError_t begin(Arena &arena, uint8_t *cur) {
        uint64_t *d_shift = nullptr;  // (the arena frees it)
        hipError_t e;
        if ((e = arena.take(&d_shift, job.n * 8)) != hipSuccess || (e = hipMemcpyAsync(d_shift, job.shift, job.n * 8, hipMemcpyHostToDevice, job.stream)) != hipSuccess) return e;
        inputs.shift = d_shift;
        for (uint32_t i = 0; i < job.n; ++i) {
            const uint64_t rows = job.first[i + 1] - job.first[i];
            if (rows && (e = hipMemsetAsync(cur + job.first[i], int(i), rows, job.stream)) != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // where the tiles of `src` start in every input
    hipError_t tile_starts(const uint8_t *src) const {
        const uint64_t ncounts = uint64_t(job.n) * job.ntiles;
        hipLaunchKernelGGL(k_many_input_counts, dim3(tile_grid), dim3(kThreads), 0, job.stream, src, job.total, job.n, job.ntiles, job.d_counts);
        return exclusive_scan(job.d_counts, ncounts, job.d_counts + ncounts, job.stream);
    }
    void histogram() const {
        hipLaunchKernelGGL(k_many_histogram, dim3(tile_grid), dim3(kThreads), 0, job.stream, job.d_counts, inputs, job.ntiles, job.d_hist);
    }
    hipError_t scatter(const uint8_t *cur, uint8_t *next) const {
        hipLaunchKernelGGL(k_many_scatter, dim3(tile_grid), dim3(kThreads), 0, job.stream, cur, job.d_counts, inputs, job.ntiles, job.d_hist, next, job.d_flag);
        return hipSuccess;
    }
    void emit(const uint8_t *src, uint8_t *merged) const {
        hipLaunchKernelGGL(k_many_emit, dim3(tile_grid), dim3(kThreads), 0, job.stream, src, job.d_counts, inputs, job.ntiles, merged);
    }
};

}  // namespace

// ---- host side ----

uint64_t plan_merge_many(uint64_t total) {
    // the largest of the stages: decode = RLE bytes (at most a byte per symbol) + symbols + the long runs' list; iterate = symbols
    // + two arrays + (n + 6) counts per tile with their scans' scratch; emit = symbols + the array + merged symbols; encode =
    // merged symbols + the array + RLE bytes.  Three bytes per symbol cover the arrays; the counts are at most 38 x 8 bytes per
    // kMergeTile rows whatever n is, under a thirteenth of a byte per symbol, and an eighth covers them, their scratch and every
    // list; 8 MiB the allocations' rounding and the inputs' padding.
    return 3 * total + total / 8 + (8ull << 20);
}

hipError_t merge_rle_many(const MergeSpan *spans, size_t n, hipStream_t stream, MergeOutput *out) { return run_merge<ByteState>(spans, n, stream, out); }

}  // namespace msbwt
