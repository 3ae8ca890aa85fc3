// Construction: the multi-string BWT of a read set, built on the device (the reference: DynamicBWT::create_from_fastx,
// src/dynamic_bwt.rs:453-473; the semantics: naive_bwt, src/bwt_util.rs:154-171).
//
// The text is every read followed by '$' (code 0), the reads in lexicographic order; row i of the BWT is the symbol before the
// i-th smallest suffix, '$' < A < C < G < N < T, two suffixes that are equal up to and including their '$' in text order.
//
//   1. read order   the n suffixes at read starts are sorted by the sort of step 3 (one piece); a scan of their lengths gives
//                   every read its place in the text, which is written one byte per symbol.  A bitmap marks the '$'s.
//   2. pieces       a histogram of all suffixes by their first four symbols (4096 bins, zero after the suffix's own '$');
//                   the host cuts the bins into pieces of at most `piece_limit` suffixes (a larger bin is a piece of its own).
//   3. sort         a piece's positions are collected in text order (count, scan, compact), then sorted by 63-bit key words of
//                   21 symbols at 3 bits, zero after the suffix's own '$', from the last word the longest read reaches down to
//                   word 0.  A word is gathered from the text for the current permutation and sorted by 8 stable 8-bit
//                   radix passes (radix_sort.hip: per-tile digit histogram, scan, scatter).  Stable passes over keys that are
//                   equal exactly where the suffixes are leave equal suffixes in text order.
//   4. emit         text[p - 1] for every sorted position p, into the piece's slot of the symbol array.
//   5. encode       the symbol array's runs -> RLE bytes (run_encode.hip, shared with the merge).
//
// Integer only; every kernel runs without scratch memory.  64-bit: every text position, offset into the symbol and
// RLE arrays, histogram bin and scanned rank.  32-bit: a suffix's rank inside its tile (< kRadixSortTile), a tile's digit
// counts, and -- while the text is below 2^32 symbols -- the stored positions themselves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

#include "radix_sort.hpp"
#include "reads_build.hpp"
#include "rle_codec.hpp"
#include "run_encode.hpp"
#include "workgroup.hpp"

namespace msbwt {

namespace {

constexpr uint32_t kThreads = kScanThreads, kWaves = kScanWaves;
constexpr uint32_t kPassesPerWord = 8;  // 8 x 8 bits cover the 63 key bits; an even number: a word's result is back where it started
constexpr uint32_t kWordSymbols = 21;
constexpr uint32_t kCollectPer = 8, kCollectTile = kThreads * kCollectPer;  // collect: text positions per thread / workgroup
constexpr uint32_t kBins = 4096;
constexpr uint32_t kPad = 128;  // zero bytes after the reads and after the text: wide loads past the last symbol stay inside
static_assert(kPassesPerWord % 2 == 0 && kPassesPerWord * kRadixDigitBits == 64, "a key word's passes");

// ---- keys ----

// up to 21 symbols from p (24 bytes readable), the first in bits 62..60; symbols from `nvalid` on read as zero
__device__ __forceinline__ uint64_t pack_word(const uint8_t *__restrict__ p, uint32_t nvalid) {
    uint64_t w[3];
    __builtin_memcpy(w, p, 24);
    uint64_t key = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWordSymbols; ++j) {
        const uint64_t s = (w[j >> 3] >> (8u * (j & 7u))) & 7ull;
        key |= j < nvalid ? s << (60u - 3u * j) : 0ull;
    }
    return key;
}

// symbols from p to the first '$' at or after it, looking no further than `limit` (a value >= limit: none before that)
__device__ __forceinline__ uint64_t terminator_distance(const uint64_t *__restrict__ bits, uint64_t p, uint64_t limit) {
    uint64_t word = p >> 6;
    const uint32_t off = uint32_t(p & 63u);
    uint64_t m = bits[word] >> off;
    if (m) return uint64_t(__ffsll((unsigned long long)m) - 1);
    uint64_t d = 64u - off;
    while (d < limit) {  // (ends at the text's last '$' at the latest)
        m = bits[++word];
        if (m) return d + uint64_t(__ffsll((unsigned long long)m) - 1);
        d += 64u;
    }
    return limit;
}

// the suffixes at read starts, before the text exists: element = read index
struct ReadSource {
    const uint8_t *reads;      // reads[0] = the first read's first symbol
    const uint64_t *offsets;   // n + 1, as the caller gave them
    __device__ __forceinline__ uint64_t word(uint64_t r, uint32_t w) const {
        const uint64_t lo = offsets[r], len = offsets[r + 1] - lo, start = uint64_t(kWordSymbols) * w;
        if (start >= len) return 0ull;
        return pack_word(reads + (lo - offsets[0]) + start, uint32_t(min(uint64_t(kWordSymbols), len - start)));
    }
};

// the suffixes of the text: element = text position
struct TextSource {
    const uint8_t *text;
    const uint64_t *terminators;  // bit p set: text[p] == '$'
    __device__ __forceinline__ uint64_t word(uint64_t p, uint32_t w) const {
        const uint64_t start = uint64_t(kWordSymbols) * w;
        const uint64_t len = terminator_distance(terminators, p, start + kWordSymbols);
        if (start >= len) return 0ull;
        return pack_word(text + p + start, uint32_t(min(uint64_t(kWordSymbols), len - start)));
    }
};

template <class Pos, class Source>
__global__ __launch_bounds__(256) void k_gather_keys(Source src, const Pos *__restrict__ pos, uint64_t n, uint32_t w, uint64_t *__restrict__ keys) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) keys[i] = src.word(uint64_t(pos[i]), w);
}

template <class Pos>
__global__ __launch_bounds__(256) void k_iota(Pos *__restrict__ pos, uint64_t n) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) pos[i] = Pos(i);
}

// ---- step 1: the text ----

__global__ __launch_bounds__(256) void k_ascii_to_codes(uint8_t *__restrict__ reads, uint64_t n) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const uint32_t c = reads[i] | 0x20u;  // string_util.rs:15-32: A/a C/c G/g T/t, anything else N
        reads[i] = uint8_t(c == 'a' ? 1u : c == 'c' ? 2u : c == 'g' ? 3u : c == 't' ? 5u : 4u);
    }
}

// spans[i] = symbols the i-th read in sorted order takes in the text, its '$' included; spans[n] = 0 (the scan leaves the total there)
template <class Pos>
__global__ __launch_bounds__(256) void k_read_spans(const Pos *__restrict__ order, const uint64_t *__restrict__ offsets, uint64_t n, uint64_t *__restrict__ spans) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= n; i += stride) {
        const uint64_t r = i < n ? uint64_t(order[i]) : 0ull;
        spans[i] = i < n ? offsets[r + 1] - offsets[r] + 1ull : 0ull;
    }
}

// one wave per read: its symbols to text[starts[i] ..), then the '$'
template <class Pos>
__global__ __launch_bounds__(256) void k_layout_text(const Pos *__restrict__ order, const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ reads,
                                                     const uint64_t *__restrict__ starts, uint64_t n, uint8_t *__restrict__ text) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = uint64_t(gridDim.x) * kWaves;
    for (uint64_t i = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6); i < n; i += nwaves) {
        const uint64_t r = uint64_t(order[i]), lo = offsets[r], len = offsets[r + 1] - lo, to = starts[i];
        const uint8_t *src = reads + (lo - offsets[0]);
        for (uint64_t j = lane; j < len; j += 64u) text[to + j] = src[j];
        if (lane == 0u) text[to + len] = 0u;
    }
}

// bit p of terminators = (text[p] == 0), one word per thread; the text is readable (zero) up to the end of its last word
__global__ __launch_bounds__(256) void k_terminator_bits(const uint8_t *__restrict__ text, uint64_t nwords, uint64_t *__restrict__ terminators) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t w = uint64_t(blockIdx.x) * kThreads + threadIdx.x; w < nwords; w += stride) {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(text + w * 64u);  // hipMalloc aligns the text
        uint64_t bits = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) {
            const uint64_t x = src[q];
#pragma unroll
            for (uint32_t b = 0; b < 8u; ++b) bits |= ((x >> (8u * b)) & 0xFFull) == 0ull ? 1ull << (q * 8u + b) : 0ull;
        }
        terminators[w] = bits;
    }
}

// ---- step 2 and 3: pieces ----

// the first four symbols of the suffix at p, zero after its own '$': 12 bits
__device__ __forceinline__ uint32_t suffix_bin(const uint8_t *__restrict__ text, uint64_t p) {
    uint32_t raw;
    __builtin_memcpy(&raw, text + p, 4);
    uint32_t bin = 0;
    bool live = true;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t s = live ? (raw >> (8u * j)) & 7u : 0u;
        live = live && s != 0u;
        bin = (bin << 3) | s;
    }
    return bin;
}

__global__ __launch_bounds__(256) void k_bin_histogram(const uint8_t *__restrict__ text, uint64_t n, unsigned long long *__restrict__ bins) {
    __shared__ uint32_t counts[kBins];
    for (uint32_t b = threadIdx.x; b < kBins; b += kThreads) counts[b] = 0u;
    __syncthreads();
    // a workgroup takes a contiguous share below 2^32 positions: n < 2^40 over at least 2^10 workgroups when n is large
    const uint64_t per = ceil_div(n, gridDim.x);
    const uint64_t lo = uint64_t(blockIdx.x) * per, hi = min(n, lo + per);
    for (uint64_t p = lo + threadIdx.x; p < hi; p += kThreads) atomicAdd(&counts[suffix_bin(text, p)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kBins; b += kThreads)
        if (counts[b]) atomicAdd(&bins[b], (unsigned long long)counts[b]);
}

// counts[tile] = the positions of [tile * kCollectTile, ...) whose bin lies in [bin_lo, bin_hi)
__global__ __launch_bounds__(256) void k_piece_count(const uint8_t *__restrict__ text, uint64_t n, uint32_t bin_lo, uint32_t bin_hi, uint64_t *__restrict__ counts) {
    __shared__ uint64_t wave_sums[kWaves];
    const uint64_t base = uint64_t(blockIdx.x) * kCollectTile + uint64_t(threadIdx.x) * kCollectPer;
    uint64_t c = 0;
#pragma unroll
    for (uint32_t i = 0; i < kCollectPer; ++i) {
        const uint32_t b = base + i < n ? suffix_bin(text, base + i) : kBins;
        c += b >= bin_lo && b < bin_hi ? 1u : 0u;
    }
    uint64_t total;
    block_exclusive_sum(c, wave_sums, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts: scanned.  pos[...] = those positions, ascending
template <class Pos>
__global__ __launch_bounds__(256) void k_piece_collect(const uint8_t *__restrict__ text, uint64_t n, uint32_t bin_lo, uint32_t bin_hi,
                                                       const uint64_t *__restrict__ counts, Pos *__restrict__ pos) {
    __shared__ uint64_t wave_sums[kWaves];
    const uint64_t base = uint64_t(blockIdx.x) * kCollectTile + uint64_t(threadIdx.x) * kCollectPer;
    uint32_t member = 0;
#pragma unroll
    for (uint32_t i = 0; i < kCollectPer; ++i) {
        const uint32_t b = base + i < n ? suffix_bin(text, base + i) : kBins;
        member |= b >= bin_lo && b < bin_hi ? 1u << i : 0u;
    }
    uint64_t total;
    uint64_t at = counts[blockIdx.x] + block_exclusive_sum(uint64_t(__popc(member)), wave_sums, &total);  // < the piece's size
#pragma unroll
    for (uint32_t i = 0; i < kCollectPer; ++i)
        if ((member >> i) & 1u) pos[at++] = Pos(base + i);
}

// ---- step 4 ----

template <class Pos>
__global__ __launch_bounds__(256) void k_emit(const uint8_t *__restrict__ text, const Pos *__restrict__ pos, uint64_t n, uint8_t *__restrict__ symbols) {
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t p = uint64_t(pos[i]);
        symbols[i] = p ? text[p - 1u] : uint8_t(0);  // before a read's first symbol stands the previous read's '$'
    }
}

// ---- host side ----

// buffers of the sort of up to `capacity` elements
template <class Pos>
struct SortBuffers {
    uint64_t capacity = 0;
    uint64_t *keys_a = nullptr, *keys_b = nullptr, *hist = nullptr, *scan = nullptr;
    Pos *pos_a = nullptr, *pos_b = nullptr;
    hipError_t take(Arena &arena, uint64_t n) {
        capacity = n;
        hipError_t e = arena.take(&keys_a, n * 8);
        if (e == hipSuccess) e = arena.take(&keys_b, n * 8);
        if (e == hipSuccess) e = arena.take(&pos_a, n * sizeof(Pos));
        if (e == hipSuccess) e = arena.take(&pos_b, n * sizeof(Pos));
        if (e == hipSuccess) e = arena.take(&hist, radix_sort_hist_words(n) * 8);
        if (e == hipSuccess) e = arena.take(&scan, radix_sort_scan_words(n) * 8);
        return e;
    }
    void give_back(Arena &arena) {
        arena.give_back(keys_a);
        arena.give_back(keys_b);
        arena.give_back(pos_a);
        arena.give_back(pos_b);
        arena.give_back(hist);
        arena.give_back(scan);
    }
};

// pos_a[0 .. n): the elements in their tie order -> the same, sorted by words [0, nwords) of their keys.  8 passes per word: the
// result of every word is back in pos_a.
template <class Pos, class Source>
hipError_t sort_elements(const Source &src, SortBuffers<Pos> &b, uint64_t n, uint32_t nwords, hipStream_t stream) {
    if (n < 2) return hipSuccess;
    for (uint32_t w = nwords; w-- > 0;) {
        hipLaunchKernelGGL((k_gather_keys<Pos, Source>), dim3(capped_grid(n, kThreads)), dim3(kThreads), 0, stream, src, b.pos_a, n, w, b.keys_a);
        bool in_b = false;  // (never: an even number of passes)
        const hipError_t e = radix_sort_passes(b.keys_a, b.pos_a, b.keys_b, b.pos_b, n, 0, kPassesPerWord, b.hist, b.scan, nullptr, stream, &in_b);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

struct Piece {
    uint32_t bin_lo, bin_hi;
    uint64_t count, offset;
    bool sort;  // false: one bin of suffixes shorter than four symbols (all the same suffix) or a single suffix -- text order is the order
};

std::vector<Piece> cut_pieces(const std::vector<uint64_t> &bins, uint64_t limit) {
    std::vector<Piece> pieces;
    uint64_t offset = 0;
    for (uint32_t b = 0; b < kBins;) {
        Piece p{b, b + 1, bins[b], offset, false};
        while (p.bin_hi < kBins && p.count + bins[p.bin_hi] <= limit) p.count += bins[p.bin_hi++];
        uint32_t occupied = 0;
        bool four = false;  // an occupied bin whose four symbols are all letters
        for (uint32_t i = p.bin_lo; i < p.bin_hi; ++i) {
            if (!bins[i]) continue;
            ++occupied;
            four = four || ((i & 7u) && ((i >> 3) & 7u) && ((i >> 6) & 7u) && (i >> 9));
        }
        p.sort = occupied > 1 || (four && p.count > 1);
        if (p.count) pieces.push_back(p);
        offset += p.count;
        b = p.bin_hi;
    }
    return pieces;
}

template <class Pos>
hipError_t build(const uint8_t *reads, const uint64_t *offsets, uint64_t n, bool ascii, uint64_t piece_limit, hipStream_t stream, ReadsBuildOutput *out) {
    Arena arena;
    auto clock = std::chrono::steady_clock::now();
    hipError_t e = hipSuccess;
    auto failed = [&](const char *what) {
        out->what = what;
        return e;
    };
    // a stage ends: the stream drained, the time booked
    auto lap = [&](ReadsBuildStage stage) {
        const hipError_t s = hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        out->stage_ms[stage] += std::chrono::duration<double, std::milli>(now - clock).count();
        clock = now;
        return s;
    };
    const uint64_t nbytes = offsets[n] - offsets[0], total = nbytes + n;
    uint64_t longest = 0;
    for (uint64_t r = 0; r < n; ++r) longest = std::max(longest, offsets[r + 1] - offsets[r]);
    const uint32_t nwords = uint32_t(ceil_div(longest, kWordSymbols));

    // ---- the reads in HBM
    uint8_t *d_reads = nullptr, *d_text = nullptr;
    uint64_t *d_offsets = nullptr;
    if ((e = arena.take(&d_reads, nbytes + kPad)) != hipSuccess || (e = arena.take(&d_offsets, (n + 1) * 8)) != hipSuccess) return failed("the reads in HBM");
    if (nbytes) e = hipMemcpyAsync(d_reads, reads + offsets[0], nbytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_reads + nbytes, 0, kPad, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_offsets, offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = lap(kStageCopyIn);
    if (e != hipSuccess) return failed("copying the reads to HBM");
    if (ascii && nbytes) hipLaunchKernelGGL(k_ascii_to_codes, dim3(capped_grid(nbytes, kThreads)), dim3(kThreads), 0, stream, d_reads, nbytes);

    // ---- 1. the reads' order, the text
    const uint64_t text_bytes = ceil_div(total, 64) * 64 + kPad, bitmap_words = ceil_div(total, 64);
    {
        SortBuffers<Pos> sb;
        uint64_t *d_starts = nullptr;
        if ((e = sb.take(arena, n)) != hipSuccess || (e = arena.take(&d_starts, (n + 1) * 8 + scan_scratch_words(n + 1) * 8)) != hipSuccess ||
            (e = arena.take(&d_text, text_bytes)) != hipSuccess)
            return failed("the buffers of the read order");
        hipLaunchKernelGGL((k_iota<Pos>), dim3(capped_grid(n, kThreads)), dim3(kThreads), 0, stream, sb.pos_a, n);
        if ((e = sort_elements(ReadSource{d_reads, d_offsets}, sb, n, nwords, stream)) != hipSuccess) return failed("sorting the reads");
        hipLaunchKernelGGL((k_read_spans<Pos>), dim3(capped_grid(n + 1, kThreads)), dim3(kThreads), 0, stream, sb.pos_a, d_offsets, n, d_starts);
        if ((e = exclusive_scan(d_starts, n + 1, d_starts + n + 1, stream)) != hipSuccess) return failed("placing the reads");
        if ((e = hipMemsetAsync(d_text + total, 0, text_bytes - total, stream)) != hipSuccess) return failed("clearing the text's padding");
        hipLaunchKernelGGL((k_layout_text<Pos>), dim3(capped_grid(n, kWaves)), dim3(kThreads), 0, stream, sb.pos_a, d_offsets, d_reads, d_starts, n, d_text);
        if ((e = hipGetLastError()) != hipSuccess || (e = lap(kStageReadOrder)) != hipSuccess) return failed("laying out the text");
        sb.give_back(arena);
        arena.give_back(d_starts);
        arena.give_back(d_reads);
        arena.give_back(d_offsets);
    }

    // ---- 2. terminators, histogram, pieces
    uint64_t *d_terminators = nullptr;
    unsigned long long *d_bins = nullptr;
    if ((e = arena.take(&d_terminators, bitmap_words * 8)) != hipSuccess || (e = arena.take(&d_bins, kBins * 8)) != hipSuccess) return failed("the terminator bitmap");
    std::vector<uint64_t> bins(kBins);
    hipLaunchKernelGGL(k_terminator_bits, dim3(capped_grid(bitmap_words, kThreads)), dim3(kThreads), 0, stream, d_text, bitmap_words, d_terminators);
    if ((e = hipMemsetAsync(d_bins, 0, kBins * 8, stream)) != hipSuccess) return failed("clearing the histogram");
    hipLaunchKernelGGL(k_bin_histogram, dim3(capped_grid(total, kBins, 1024)), dim3(kThreads), 0, stream, d_text, total, d_bins);
    if ((e = hipMemcpyAsync(bins.data(), d_bins, kBins * 8, hipMemcpyDeviceToHost, stream)) != hipSuccess || (e = lap(kStageHistogram)) != hipSuccess)
        return failed("the histogram of the suffixes");
    arena.give_back(d_bins);
    const std::vector<Piece> pieces = cut_pieces(bins, piece_limit);
    uint64_t largest = 0;
    for (const Piece &p : pieces) largest = std::max(largest, p.count);
    out->pieces = pieces.size();
    out->largest_piece = largest;

    // ---- 3 and 4. piece by piece
    uint8_t *d_symbols = nullptr;
    uint64_t *d_counts = nullptr;
    const uint64_t collect_tiles = ceil_div(total, kCollectTile);
    SortBuffers<Pos> sb;
    if ((e = arena.take(&d_symbols, total)) != hipSuccess || (e = arena.take(&d_counts, (collect_tiles + scan_scratch_words(collect_tiles)) * 8)) != hipSuccess)
        return failed("the symbol array");
    if ((e = sb.take(arena, largest)) != hipSuccess) {
        out->what = "the sort buffers of a piece of " + std::to_string(largest) + " suffixes do not fit the free HBM (piece limit " + std::to_string(piece_limit) +
                    ": lower it)";
        return e;
    }
    const TextSource source{d_text, d_terminators};
    for (const Piece &p : pieces) {
        hipLaunchKernelGGL(k_piece_count, dim3(uint32_t(collect_tiles)), dim3(kThreads), 0, stream, d_text, total, p.bin_lo, p.bin_hi, d_counts);
        if ((e = exclusive_scan(d_counts, collect_tiles, d_counts + collect_tiles, stream)) != hipSuccess) return failed("collecting a piece");
        hipLaunchKernelGGL((k_piece_collect<Pos>), dim3(uint32_t(collect_tiles)), dim3(kThreads), 0, stream, d_text, total, p.bin_lo, p.bin_hi, d_counts, sb.pos_a);
        if ((e = hipGetLastError()) != hipSuccess || (e = lap(kStageCollect)) != hipSuccess) return failed("collecting a piece");
        if (p.sort && (e = sort_elements(source, sb, p.count, nwords, stream)) != hipSuccess) return failed("sorting a piece");
        if ((e = lap(kStageSort)) != hipSuccess) return failed("sorting a piece");
        hipLaunchKernelGGL((k_emit<Pos>), dim3(capped_grid(p.count, kThreads)), dim3(kThreads), 0, stream, d_text, sb.pos_a, p.count, d_symbols + p.offset);
        if ((e = hipGetLastError()) != hipSuccess || (e = lap(kStageEmit)) != hipSuccess) return failed("emitting a piece");
    }
    sb.give_back(arena);
    arena.give_back(d_counts);
    arena.give_back(d_terminators);
    arena.give_back(d_text);

    // ---- 5. encode
    uint8_t *d_rle = nullptr;
    uint64_t need = 0;
    const char *step = "";
    if ((e = encode_symbol_runs(arena, d_symbols, total, stream, &d_rle, &need, &step)) != hipSuccess) return failed(step);
    if ((e = lap(kStageEncode)) != hipSuccess) return failed("writing the runs");
    out->d_rle = arena.keep(d_rle);
    out->rle_bytes = need;
    return hipSuccess;
}

}  // namespace

ReadsBuildPlan plan_reads_build(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t piece) {
    // resident: text and symbols (or reads and text) at one byte each, the terminator bitmap, the collect counts; per suffix of a
    // piece: two key and two position arrays (64-bit positions assumed) and its share of the tile histograms
    constexpr uint64_t kPerSuffix = 2 * (8 + 8) + 1, kMaxPiece = kMaxSymbols;
    const uint64_t resident = 2 * total_symbols + total_symbols / 8 + total_symbols / 128 + (1ull << 20);
    const uint64_t usable = free_hbm_bytes - free_hbm_bytes / 10;
    ReadsBuildPlan p;
    p.auto_piece = usable > resident ? std::min(kMaxPiece, std::max<uint64_t>(1, (usable - resident) / kPerSuffix)) : 1;
    const uint64_t in_force = std::min(piece ? std::min(piece, kMaxPiece) : p.auto_piece, std::max<uint64_t>(total_symbols, 1));
    p.device_bytes = resident + in_force * kPerSuffix;
    return p;
}

hipError_t build_rle_from_reads(const uint8_t *reads, const uint64_t *offsets, uint64_t n, bool ascii, uint64_t piece_limit, bool wide, hipStream_t stream,
                                ReadsBuildOutput *out) {
    const uint64_t total = offsets[n] - offsets[0] + n;
    if (n == 0 || piece_limit == 0) return hipErrorInvalidValue;
    if (wide || total >= (1ull << 32)) return build<uint64_t>(reads, offsets, n, ascii, piece_limit, stream, out);
    return build<uint32_t>(reads, offsets, n, ascii, piece_limit, stream, out);
}

}  // namespace msbwt
