// Merge: the BWTs of two read sets -> the BWT of their union, without the reads (Holt & McMillan 2014; the reference:
// bwt_util::pairwise_bwt_merge, src/bwt_util.rs:21-141).
//
// The state is one bit per merged row: set = the row is input 1's.  It starts as input 0's rows, then input 1's.  One iteration
// reads the rows' symbols in the order the vector gives and sends every row's bit to (rows with a smaller symbol) + (rows with the
// same symbol before it): a stable six-way counting sort of the vector by symbol.  When an iteration changes nothing the vector is
// the interleave of the union's BWT; rows of equal rotations stay input 0's first, because the sort is stable and they started so.
//
//   1. decode    both RLE streams -> one byte per symbol.  Every RLE byte is a sub-run of digit << 5 * (its index in its run)
//                symbols (rle_subruns.hpp: the walk of the index loader, 16 bytes per thread, every input at a 16-byte border);
//                a tile's sub-run sum, a scan, and every thread knows where its sub-runs start.  Sub-runs below 1024
//                symbols are written by their thread, longer ones are cut into pieces of at most 2^20 symbols on a list that a
//                second kernel fills with 16-byte stores, a workgroup per piece.
//   2. iterate   tiles of kMergeTile rows.  a) set bits per tile, scan: where the tile's rows start in either input (inside a
//                tile the rows of one input are a contiguous slice of it: the loads coalesce).  b) the tile's six symbol counts
//                (of the two slices as they lie: counts do not depend on the rows' order), symbol-major, one scan over
//                6 x tiles: the scanned counts are the bit offsets.  c) per tile and symbol the bits
//                are strung together in LDS at the alignment of their place in the next vector and written there: interior words
//                with plain stores, the first and the last word, which neighbouring segments share, with atomicOr into zeroes.
//                d) compare the two vectors, one word back to the host.
//   3. emit      the merged symbols, through the final vector.
//   4. encode    run_encode.hip, as the builder from reads.
//
// Integer only; every kernel runs without scratch memory.  Every row index, tile offset and bit offset is 64-bit; 32-bit are
// counts and ranks inside one tile (<= kMergeTile).
#include "merge_common.hpp"

namespace msbwt {

namespace {

constexpr uint32_t kTileWords = kMergeTile / 64;       // words of the vector per tile
constexpr uint32_t kDecodePer = 16, kDecodeTile = kThreads * kDecodePer;  // decode: RLE bytes per thread / workgroup
constexpr uint64_t kShortRun = 1024;                   // sub-runs below this are written by their thread
constexpr uint64_t kPiece = 1ull << 20;                // symbols per entry of the long sub-runs' list
constexpr uint32_t kStringWords = kTileWords + 2;      // u64 words of one symbol's bit string: 63 bits of alignment + kMergeTile bits
static_assert(kDecodePer == 16, "a thread decodes what rle_subruns.hpp loads");
static_assert(kRowsPer == 16 && kTileWords == 64, "a thread holds a quarter word of the vector; wave 0 scans the tile's words");

// entries a sub-run of `value` symbols takes on the list
__host__ __device__ inline uint64_t pieces_of(uint64_t value) { return value < kShortRun ? 0ull : ceil_div(value, kPiece); }

// ---- 1. decode ----

struct Piece {
    uint64_t pos;
    uint32_t len, sym;
};

// the sub-runs of the thread's kDecodePer bytes.  The walk's error bits are not looked at: scan_merge_input has refused a stream
// that would set one before anything is copied.
__device__ __forceinline__ ThreadBytes decode_bytes(const uint8_t *__restrict__ rle, uint64_t n) {
    return load_thread_bytes(rle, n, uint64_t(blockIdx.x) * kDecodeTile + uint64_t(threadIdx.x) * kDecodePer);
}

__global__ __launch_bounds__(256) void k_decode_sums(const uint8_t *__restrict__ rle, uint64_t n, uint64_t *__restrict__ sums) {
    __shared__ uint64_t wave_sums[kScanWaves];
    const ThreadBytes tb = decode_bytes(rle, n);
    uint64_t mine = 0;
    (void)for_each_subrun(tb, [&](uint32_t, uint64_t v) { mine += v; });
    uint64_t total;
    block_exclusive_sum(mine, wave_sums, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: scanned.  cursor: entries of the list taken so far.
__global__ __launch_bounds__(256) void k_decode_paint(const uint8_t *__restrict__ rle, uint64_t n, const uint64_t *__restrict__ sums, uint8_t *__restrict__ symbols,
                                                      uint64_t total, Piece *__restrict__ pieces, uint64_t capacity, unsigned long long *__restrict__ cursor) {
    __shared__ uint64_t wave_sums[kScanWaves];
    const ThreadBytes tb = decode_bytes(rle, n);
    uint64_t mine = 0;
    (void)for_each_subrun(tb, [&](uint32_t, uint64_t v) { mine += v; });
    uint64_t all;
    uint64_t pos = sums[blockIdx.x] + block_exclusive_sum(mine, wave_sums, &all);
    (void)for_each_subrun(tb, [&](uint32_t sym, uint64_t v) {
        if (v < kShortRun) {
            for (uint64_t k = 0; k < v && pos + k < total; ++k) symbols[pos + k] = uint8_t(sym);
        } else {
            const uint64_t count = pieces_of(v), slot = atomicAdd(cursor, (unsigned long long)count);
            for (uint64_t q = 0; q < count && slot + q < capacity; ++q)
                pieces[slot + q] = Piece{pos + q * kPiece, uint32_t(min(kPiece, v - q * kPiece)), sym};
        }
        pos += v;
    });
}

// a workgroup per piece: bytes up to the first 16-byte border, 16-byte stores, the bytes after the last border
__global__ __launch_bounds__(256) void k_decode_fill(const Piece *__restrict__ pieces, uint64_t npieces, uint8_t *__restrict__ symbols, uint64_t total) {
    for (uint64_t p = blockIdx.x; p < npieces; p += gridDim.x) {
        const Piece piece = pieces[p];
        const uint64_t lo = piece.pos, hi = min(total, lo + piece.len);
        if (lo >= hi) continue;
        const uint64_t body_lo = min(hi, (lo + 15u) & ~15ull), body_hi = max(body_lo, hi & ~15ull);
        const uint32_t word = piece.sym * 0x01010101u;
        if (lo + threadIdx.x < body_lo) symbols[lo + threadIdx.x] = uint8_t(piece.sym);
        for (uint64_t x = body_lo + uint64_t(threadIdx.x) * 16u; x < body_hi; x += kThreads * 16u)
            *reinterpret_cast<uint4 *>(symbols + x) = make_uint4(word, word, word, word);  // hipMalloc aligns the array
        if (body_hi + threadIdx.x < hi) symbols[body_hi + threadIdx.x] = uint8_t(piece.sym);
    }
}

// ---- 2. iterate ----

// word w of the first vector: rows [t0, total) are input 1's; the bits past the last row stay zero, in every vector
__global__ __launch_bounds__(256) void k_first_vector(uint64_t *__restrict__ bits, uint64_t nwords, uint64_t t0, uint64_t total) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t w = uint64_t(blockIdx.x) * kThreads + threadIdx.x; w < nwords; w += stride) {
        const uint64_t lo = w * 64u;
        uint64_t v = 0;
        if (lo + 64u > t0 && lo < total) {
            v = ~0ull;
            if (t0 > lo) v &= ~0ull << (t0 - lo);
            if (total < lo + 64u) v &= ~0ull >> (lo + 64u - total);
        }
        bits[w] = v;
    }
}

// ones[tile] = set bits of the tile, a wave per tile
__global__ __launch_bounds__(256) void k_tile_ones(const uint64_t *__restrict__ bits, uint64_t nwords, uint64_t ntiles, uint64_t *__restrict__ ones) {
    const uint64_t tile = uint64_t(blockIdx.x) * kScanWaves + (threadIdx.x >> 6), w = tile * kTileWords + (threadIdx.x & 63u);
    const uint32_t c = wave_sum(w < nwords ? uint32_t(__popcll(bits[w])) : 0u);
    if ((threadIdx.x & 63u) == 0u && tile < ntiles) ones[tile] = c;
}

struct TileShared {
    uint64_t words[kTileWords];   // the tile's words of the vector
    uint32_t before[kTileWords];  // set bits of the tile before each word
    uint32_t ones;
    uint8_t stage[kMergeTile];    // the tile's symbols: input 0's slice, then input 1's
};

struct Inputs {
    const uint8_t *sym0, *sym1;
    uint64_t t0, t1;
};

// a thread's kRowsPer consecutive rows
struct Rows {
    uint64_t syms;  // 3 bits each, kNoRow past the last row
    uint32_t bits;  // bit j: row j is input 1's
};

// symbol k of a tile's rows taken input by input: input 0's slice [start0, start0 + n0), then input 1's from start1 on.  The
// load itself is unconditional (of element 0 when the index is past the input, which it is not while the vector has exactly t1
// set bits; element 0 of an empty input is a byte of the symbol array or of the slack run_merge allocates past it), so that a
// thread's loads are all in flight at once.
__device__ __forceinline__ uint32_t slice_symbol(const Inputs &in, uint64_t start0, uint64_t start1, uint32_t n0, uint32_t k) {
    const bool first = k < n0;
    const uint64_t i = first ? start0 + k : start1 + (k - n0);
    const bool inside = i < (first ? in.t0 : in.t1);
    const uint32_t s = (first ? in.sym0 : in.sym1)[inside ? i : 0ull];
    return inside ? s : kNoRow;
}

// ones_before: scanned.  Every thread of the workgroup calls it, once.
__device__ __forceinline__ Rows load_rows(TileShared &sh, const uint64_t *__restrict__ bits, uint64_t nwords, const uint64_t *__restrict__ ones_before,
                                          const Inputs &in) {
    const uint32_t t = threadIdx.x;
    const uint64_t tile = blockIdx.x, base = tile * kMergeTile, total = in.t0 + in.t1;
    if (t < kTileWords) {  // wave 0
        const uint64_t wi = tile * kTileWords + t, w = wi < nwords ? bits[wi] : 0ull;
        const uint32_t c = uint32_t(__popcll(w)), incl = wave_inclusive_sum(c);
        sh.words[t] = w;
        sh.before[t] = incl - c;
        if (t == 63u) sh.ones = incl;
    }
    __syncthreads();
    const uint32_t valid = uint32_t(min(uint64_t(kMergeTile), total - base)), n1 = sh.ones, n0 = valid - n1;
    const uint64_t start1 = ones_before[tile], start0 = base - start1;
#pragma unroll
    for (uint32_t r = 0; r < kRowsPer; ++r) sh.stage[r * kThreads + t] = uint8_t(slice_symbol(in, start0, start1, n0, r * kThreads + t));  // (past `valid`: not read)
    __syncthreads();
    const uint64_t w = sh.words[t >> 2];
    const uint32_t q = (t & 3u) * kRowsPer;
    Rows r;
    r.bits = uint32_t(w >> q) & 0xFFFFu;
    r.syms = 0;
    uint32_t o = sh.before[t >> 2] + uint32_t(__popcll(w & ((1ull << q) - 1ull)));
    uint32_t z = t * kRowsPer - o;
    o += n0;
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) {
        const uint32_t b = (r.bits >> j) & 1u, at = (b ? o : z) & (kMergeTile - 1u);
        o += b;
        z += 1u - b;
        const uint32_t s = t * kRowsPer + j < valid ? sh.stage[at] : kNoRow;
        r.syms |= uint64_t(s) << (3u * j);
    }
    return r;
}

// hist[symbol * ntiles + tile] = the tile's rows with that symbol.  The counts do not depend on the order of the rows inside
// the tile, so the two slices are counted as they lie; ones_before (scanned) says where they start and end.
__global__ __launch_bounds__(256) void k_tile_histogram(const uint64_t *__restrict__ ones_before, Inputs in, uint64_t ntiles, uint64_t *__restrict__ hist) {
    __shared__ uint64_t wave_sums[kScanWaves];
    const uint64_t tile = blockIdx.x, base = tile * kMergeTile;
    const uint32_t valid = uint32_t(min(uint64_t(kMergeTile), in.t0 + in.t1 - base));
    const uint64_t start1 = ones_before[tile], end1 = tile + 1u < ntiles ? ones_before[tile + 1u] : in.t1, start0 = base - start1;
    const uint32_t n0 = valid - uint32_t(end1 - start1);
    uint64_t a = 0, b = 0, all_a, all_b;
#pragma unroll
    for (uint32_t r = 0; r < kRowsPer; ++r) {
        const uint32_t k = r * kThreads + threadIdx.x, s = slice_symbol(in, start0, start1, n0, k);
        count_symbol(k < valid ? s : kNoRow, &a, &b);
    }
    block_exclusive_sum(a, wave_sums, &all_a);
    block_exclusive_sum(b, wave_sums, &all_b);
    if (threadIdx.x < kSymbols) hist[uint64_t(threadIdx.x) * ntiles + blockIdx.x] = field(all_a, all_b, threadIdx.x);
}

// hist: scanned.  next: zero.
__global__ __launch_bounds__(256) void k_scatter(const uint64_t *__restrict__ bits, uint64_t nwords, const uint64_t *__restrict__ ones_before, Inputs in,
                                                 uint64_t ntiles, const uint64_t *__restrict__ hist, uint64_t *__restrict__ next) {
    __shared__ TileShared sh;
    __shared__ uint64_t wave_sums[kScanWaves];
    __shared__ uint64_t strings[kSymbols][kStringWords];
    __shared__ uint64_t offsets[kSymbols];
    for (uint32_t i = threadIdx.x; i < kSymbols * kStringWords; i += kThreads) (&strings[0][0])[i] = 0ull;
    if (threadIdx.x < kSymbols) offsets[threadIdx.x] = hist[uint64_t(threadIdx.x) * ntiles + blockIdx.x];
    const Rows r = load_rows(sh, bits, nwords, ones_before, in);  // (its barriers publish the zeroes and the offsets)
    uint64_t a = 0, b = 0, all_a, all_b;
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) count_symbol(uint32_t(r.syms >> (3u * j)) & 7u, &a, &b);
    const uint64_t before_a = block_exclusive_sum(a, wave_sums, &all_a), before_b = block_exclusive_sum(b, wave_sums, &all_b);
#pragma unroll
    for (uint32_t s = 0; s < kSymbols; ++s) {
        uint32_t v = 0, n = 0;  // the bits of the thread's rows with symbol s, in row order
#pragma unroll
        for (uint32_t j = 0; j < kRowsPer; ++j) {
            const uint32_t m = (uint32_t(r.syms >> (3u * j)) & 7u) == s ? 1u : 0u;
            v |= (m & (r.bits >> j)) << n;
            n += m;
        }
        if (v) {
            const uint32_t at = uint32_t(offsets[s] & 63u) + field(before_a, before_b, s);  // + 16 <= 63 + kMergeTile
            const uint64_t wide = uint64_t(v) << (at & 31u);
            uint32_t *words = reinterpret_cast<uint32_t *>(strings[s]);
            atomicOr(&words[at >> 5], uint32_t(wide));
            if (wide >> 32) atomicOr(&words[(at >> 5) + 1u], uint32_t(wide >> 32));
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < kSymbols; ++s) {
        const uint32_t count = field(all_a, all_b, s);
        if (count == 0u) continue;
        const uint64_t word0 = offsets[s] >> 6;
        const uint32_t nw = (uint32_t(offsets[s] & 63u) + count + 63u) >> 6;
        for (uint32_t j = threadIdx.x; j < nw; j += kThreads) {
            if (word0 + j >= nwords) continue;  // (cannot be: the scanned counts end at the last row)
            const uint64_t v = strings[s][j];
            if (j == 0u || j + 1u == nw) {
                if (v) atomicOr(reinterpret_cast<unsigned long long *>(next + word0 + j), (unsigned long long)v);
            } else {
                next[word0 + j] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_differs(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, uint64_t nwords, uint32_t *__restrict__ flag) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    bool differs = false;
    for (uint64_t w = uint64_t(blockIdx.x) * kThreads + threadIdx.x; w < nwords; w += stride) differs = differs || a[w] != b[w];
    if (differs) *flag = 1u;
}

// ---- 3. emit ----

// merged: whole tiles
__global__ __launch_bounds__(256) void k_emit_rows(const uint64_t *__restrict__ bits, uint64_t nwords, const uint64_t *__restrict__ ones_before, Inputs in,
                                                   uint8_t *__restrict__ merged) {
    __shared__ TileShared sh;
    const Rows r = load_rows(sh, bits, nwords, ones_before, in);
    *reinterpret_cast<uint4 *>(merged + uint64_t(blockIdx.x) * kMergeTile + uint64_t(threadIdx.x) * kRowsPer) = merged_symbols(r.syms);
}

// ---- the bit state under run_merge ----

struct BitState {
    using Word = uint64_t;
    static uint64_t plan(const MergeJob &job) { return plan_merge(job.first[1], job.total - job.first[1]); }
    static uint64_t state_bytes(const MergeJob &job) { return ceil_div(job.total, 64) * 8; }
    static uint64_t out_bytes(const MergeJob &job) { return ceil_div(job.total, 8); }
    static uint64_t counts(const MergeJob &) { return 1; }  // the tile's set bits

    const MergeJob &job;
    const uint64_t nwords;
    const Inputs inputs;
    const uint32_t word_grid, tile_grid;
    explicit BitState(const MergeJob &j)
        : job(j), nwords(ceil_div(j.total, 64)), inputs{j.d_sym + j.shift[0], j.d_sym + j.first[1] + j.shift[1], j.first[1], j.total - j.first[1]},
          word_grid(capped_grid(nwords, kThreads * 4u)), tile_grid(uint32_t(j.ntiles)) {}

    hipError_t begin(Arena &, uint64_t *cur) const {
        hipLaunchKernelGGL(k_first_vector, dim3(word_grid), dim3(kThreads), 0, job.stream, cur, nwords, inputs.t0, job.total);
        return hipSuccess;
    }
    // where the tiles of `bits` start in input 1
    hipError_t tile_starts(const uint64_t *bits) const {
        hipLaunchKernelGGL(k_tile_ones, dim3(uint32_t(ceil_div(job.ntiles, kScanWaves))), dim3(kThreads), 0, job.stream, bits, nwords, job.ntiles, job.d_counts);
        return exclusive_scan(job.d_counts, job.ntiles, job.d_counts + job.ntiles, job.stream);
    }
    void histogram() const {
        hipLaunchKernelGGL(k_tile_histogram, dim3(tile_grid), dim3(kThreads), 0, job.stream, job.d_counts, inputs, job.ntiles, job.d_hist);
    }
    hipError_t scatter(const uint64_t *cur, uint64_t *next) const {
        const hipError_t e = hipMemsetAsync(next, 0, nwords * 8, job.stream);  // segments share their first and last word: they are or-ed in
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_scatter, dim3(tile_grid), dim3(kThreads), 0, job.stream, cur, nwords, job.d_counts, inputs, job.ntiles, job.d_hist, next);
        hipLaunchKernelGGL(k_differs, dim3(word_grid), dim3(kThreads), 0, job.stream, cur, next, nwords, job.d_flag);
        return hipSuccess;
    }
    void emit(const uint64_t *bits, uint8_t *merged) const {
        hipLaunchKernelGGL(k_emit_rows, dim3(tile_grid), dim3(kThreads), 0, job.stream, bits, nwords, job.d_counts, inputs, merged);
    }
};

}  // namespace

// ---- host side ----

hipError_t decode(Arena &arena, const uint8_t *d_rle, uint64_t n, const MergeInput &in, uint8_t *d_symbols, hipStream_t stream, const char **what) {
    if (n == 0 || in.total == 0) return hipSuccess;
    const uint64_t tiles = ceil_div(n, kDecodeTile);
    uint64_t *d_sums = nullptr;
    Piece *d_pieces = nullptr;
    unsigned long long *d_cursor = nullptr, taken = 0;
    hipError_t e;
    *what = "the buffers of the decoder";
    if ((e = arena.take(&d_sums, (tiles + scan_scratch_words(tiles)) * 8)) != hipSuccess || (e = arena.take(&d_pieces, in.long_pieces * sizeof(Piece))) != hipSuccess ||
        (e = arena.take(&d_cursor, 8)) != hipSuccess)
        return e;
    *what = "decoding an input";
    if ((e = hipMemsetAsync(d_cursor, 0, 8, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode_sums, dim3(uint32_t(tiles)), dim3(kThreads), 0, stream, d_rle, n, d_sums);
    if ((e = exclusive_scan(d_sums, tiles, d_sums + tiles, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode_paint, dim3(uint32_t(tiles)), dim3(kThreads), 0, stream, d_rle, n, d_sums, d_symbols, in.total, d_pieces, in.long_pieces, d_cursor);
    if (in.long_pieces)
        hipLaunchKernelGGL(k_decode_fill, dim3(capped_grid(in.long_pieces, 1, 1u << 16)), dim3(kThreads), 0, stream, d_pieces, in.long_pieces, d_symbols, in.total);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpyAsync(&taken, d_cursor, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess)
        return e;
    if (taken != in.long_pieces) {
        *what = "the decoder's list of long runs does not match the host's count (a bug)";
        return hipErrorUnknown;
    }
    arena.give_back(d_sums);
    arena.give_back(d_pieces);
    arena.give_back(d_cursor);
    return hipSuccess;
}

MergeInputStatus scan_merge_input(const uint8_t *rle, size_t n, MergeInput *out) {
    uint64_t total = 0, pieces = 0;
    uint32_t prev = 8;
    int e = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t sym = rle[i] & 7u, digit = rle[i] >> 3;
        if (sym >= kSymbols) return MergeInputStatus::kInvalidSymbol;
        e = next_exponent(e, sym == prev);
        prev = sym;
        if (subrun_too_large(digit, e)) return MergeInputStatus::kTooLarge;
        const uint64_t value = subrun_value(digit, e);
        total += value;  // < 2^41
        if (total >= kMaxSymbols) return MergeInputStatus::kTooLarge;
        pieces += pieces_of(value);
    }
    out->total = total;
    out->long_pieces = pieces;
    return MergeInputStatus::kOk;
}

uint64_t plan_merge(uint64_t total0, uint64_t total1) {
    // the largest of the stages: decode = RLE bytes (at most a byte per symbol) + symbols + the long runs' list; iterate = symbols
    // + two vectors + seven counts per tile; emit and encode = merged symbols + the vector + inputs or RLE bytes.  Two bytes per
    // symbol cover the arrays, an eighth the vector, a thirty-second every list, count and scan, 8 MiB the allocations' rounding.
    const uint64_t total = total0 + total1;
    return 2 * total + total / 8 + total / 32 + (8ull << 20);
}

hipError_t merge_rle_pair(const MergeSpan *spans, size_t n, hipStream_t stream, MergeOutput *out) {
    return n == 2 ? run_merge<BitState>(spans, n, stream, out) : hipErrorInvalidValue;
}

}  // namespace msbwt
