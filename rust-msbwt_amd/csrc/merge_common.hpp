// What merge.hip (a bit per merged row, two inputs) and merge_many.hip (a byte per merged row, up to kMergeMaxInputs inputs) share,
// and nobody else includes: the constants and device helpers of the six-way counting sort, and the host side of a merge, which is
// one sequence whatever the state is -- copy in, decode, iterate until nothing changes, emit, encode.  The digit rule of the
// inputs is rle_subruns.hpp's, the bound on the rows rle_codec.hpp's kMaxSymbols, and ceil_div, capped_grid and the sums over a wave
// or a workgroup are workgroup.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>

#include "merge.hpp"
#include "rle_subruns.hpp"
#include "run_encode.hpp"
#include "workgroup.hpp"

namespace msbwt {

namespace {

constexpr uint32_t kThreads = kScanThreads;
constexpr uint32_t kRowsPer = kMergeTile / kThreads;  // consecutive rows of a tile one thread holds
constexpr uint32_t kSymbols = 6, kNoRow = 7;
constexpr uint64_t kSymbolSlack = 16;  // bytes past the last input's symbols that may be read (not used): see run_merge
static_assert(kRowsPer == 16, "a thread's rows are 16 bytes of merged symbols, of a byte state, or a quarter word of a bit state");

// one row per symbol, 16 bits each: symbols 0..3 in *a, 4 and 5 in *b (a tile's sum of a field is <= kMergeTile < 2^16)
__device__ __forceinline__ void count_symbol(uint32_t s, uint64_t *a, uint64_t *b) {
    *a += s < 4u ? 1ull << (16u * s) : 0ull;
    *b += s == 4u ? 1ull : s == 5u ? 1ull << 16 : 0ull;
}

__device__ __forceinline__ uint32_t field(uint64_t a, uint64_t b, uint32_t s) { return uint32_t((s < 4u ? a >> (16u * s) : b >> (16u * (s - 4u))) & 0xFFFFu); }

// what an emit kernel stores: a thread's kRowsPer symbols (3 bits each, kNoRow past the last row) as 16 bytes of merged symbols
__device__ __forceinline__ uint4 merged_symbols(uint64_t syms) {
    uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < kRowsPer; ++j) {
        const uint32_t s = uint32_t(syms >> (3u * j)) & 7u;
        out[j >> 2] |= (s == kNoRow ? 0u : s) << (8u * (j & 3u));
    }
    return make_uint4(out[0], out[1], out[2], out[3]);
}

// ---- host side ----

// What run_merge hands the state's kernels: where the inputs lie and the arrays every state needs.
struct MergeJob {
    hipStream_t stream = nullptr;
    uint32_t n = 0;
    uint64_t first[kMergeMaxInputs + 1] = {};  // input i's rows in the first state: [first[i], first[i + 1])
    uint64_t shift[kMergeMaxInputs] = {};      // its symbols: d_sym + first[i] + shift[i], a 16-byte border
    uint64_t total = 0, sym_bytes = 0, ntiles = 0;
    uint8_t *d_sym = nullptr;     // the decoded inputs, one after the other, kSymbolSlack readable bytes after them
    uint64_t *d_counts = nullptr; // State::counts(job) counts per tile, then their scan's scratch
    uint64_t *d_hist = nullptr;   // kSymbols counts per tile, symbol-major, then their scan's scratch
    uint32_t *d_flag = nullptr;   // zero before an iteration's kernels; they set it when the iteration changed a row
};

// The merge of n inputs that scan_merge_input accepted, 1 <= n <= kMergeMaxInputs, their totals summing to [1, 2^40).  `State`
// is what differs between a bit and a byte per merged row:
//   using Word                            the element of the two state arrays
//   static plan / state_bytes / out_bytes / counts (job)
//                                         merge.hpp's plan; bytes of one state array; of those, the bytes that describe rows;
//                                         counts per tile that tile_starts scans
//   State(job)                            when job's arrays are there
//   begin(arena, cur)                     writes the first state: input 0's rows, then input 1's, and so on
//   tile_starts(src)                      job.d_counts, scanned: where the tiles of `src` start in the inputs
//   histogram()                           job.d_hist from job.d_counts (run_merge scans it)
//   scatter(cur, next)                    `next` from `cur`, and job.d_flag
//   emit(cur, merged)                     the merged symbols through the final state
template <class State>
hipError_t run_merge(const MergeSpan *spans, size_t n, hipStream_t stream, MergeOutput *out) {
    using Word = typename State::Word;
    Arena arena;
    auto clock = std::chrono::steady_clock::now();
    hipError_t e = hipSuccess;
    if (n == 0 || n > kMergeMaxInputs) return hipErrorInvalidValue;
    MergeJob job;
    job.stream = stream;
    job.n = uint32_t(n);
    uint64_t rle_at[kMergeMaxInputs + 1];  // input i's RLE bytes in d_rle, at a 16-byte border (the decoder's loads); [n]: d_rle's size
    rle_at[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        job.first[i] = job.total;
        job.sym_bytes = (job.sym_bytes + 15u) & ~15ull;
        job.shift[i] = job.sym_bytes - job.total;
        job.sym_bytes += spans[i].in.total;
        job.total += spans[i].in.total;
        rle_at[i + 1] = (rle_at[i] + spans[i].len + 15u) & ~15ull;
    }
    job.first[n] = job.total;
    const uint64_t total = job.total;
    if (total == 0 || total >= kMaxSymbols) return hipErrorInvalidValue;
    job.ntiles = ceil_div(total, kMergeTile);
    auto failed = [&](const char *what) {
        out->what = what;
        if (e == hipErrorOutOfMemory)
            out->what += ": the merge of " + std::to_string(total) + " symbols in " + std::to_string(n) + " inputs needs " + std::to_string(State::plan(job)) + " bytes of HBM";
        return e;
    };
    auto lap = [&](MergeStage stage) {
        const hipError_t s = hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        out->stage_ms[stage] += std::chrono::duration<double, std::milli>(now - clock).count();
        clock = now;
        return s;
    };

    // ---- the RLE bytes in HBM
    uint8_t *d_rle = nullptr;
    if ((e = arena.take(&d_rle, rle_at[n])) != hipSuccess) return failed("the inputs in HBM");
    for (size_t i = 0; i < n && e == hipSuccess; ++i)
        if (spans[i].len) e = hipMemcpyAsync(d_rle + rle_at[i], spans[i].rle, spans[i].len, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = lap(kMergeCopyIn);
    if (e != hipSuccess) return failed("copying the inputs to HBM");

    // ---- 1. decode: one array, every input at a 16-byte border.  merge.hip's slice_symbol loads element 0 of an input
    // unconditionally, of an empty one too, and an empty last input begins where the array ends: kSymbolSlack bytes are allocated
    // past that end, which nobody writes and whose values nobody uses.
    const char *step = "";
    if ((e = arena.take(&job.d_sym, job.sym_bytes + kSymbolSlack)) != hipSuccess) return failed("the symbol array");
    for (size_t i = 0; i < n; ++i)
        if ((e = decode(arena, d_rle + rle_at[i], spans[i].len, spans[i].in, job.d_sym + job.first[i] + job.shift[i], stream, &step)) != hipSuccess) return failed(step);
    if ((e = lap(kMergeDecode)) != hipSuccess) return failed("decoding the inputs");
    arena.give_back(d_rle);

    // ---- 2. iterate
    Word *d_cur = nullptr, *d_next = nullptr;
    uint32_t changed = 1;
    const uint64_t ncounts = State::counts(job) * job.ntiles, nhist = kSymbols * job.ntiles;
    if ((e = arena.take(&d_cur, State::state_bytes(job))) != hipSuccess || (e = arena.take(&d_next, State::state_bytes(job))) != hipSuccess ||
        (e = arena.take(&job.d_counts, (ncounts + scan_scratch_words(ncounts)) * 8)) != hipSuccess ||
        (e = arena.take(&job.d_hist, (nhist + scan_scratch_words(nhist)) * 8)) != hipSuccess || (e = arena.take(&job.d_flag, 4)) != hipSuccess)
        return failed("the interleave arrays");
    State state(job);
    if ((e = state.begin(arena, d_cur)) != hipSuccess) return failed("the first interleave array");
    while (changed) {
        if (out->iterations >= total + 2) {  // a bug trap, nothing else: every iteration before the last settles at least one more symbol of context
            out->what = "the interleave did not settle in " + std::to_string(total + 2) + " iterations (a bug)";
            return hipErrorUnknown;
        }
        if ((e = hipMemsetAsync(job.d_flag, 0, 4, stream)) != hipSuccess || (e = state.tile_starts(d_cur)) != hipSuccess) return failed("an interleave iteration");
        state.histogram();
        if ((e = exclusive_scan(job.d_hist, nhist, job.d_hist + nhist, stream)) != hipSuccess || (e = state.scatter(d_cur, d_next)) != hipSuccess ||
            (e = hipGetLastError()) != hipSuccess || (e = hipMemcpyAsync(&changed, job.d_flag, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
            (e = hipStreamSynchronize(stream)) != hipSuccess)
            return failed("an interleave iteration");
        std::swap(d_cur, d_next);
        ++out->iterations;
    }
    if ((e = lap(kMergeIterate)) != hipSuccess) return failed("the interleave iterations");
    arena.give_back(d_next);
    arena.give_back(job.d_hist);
    arena.give_back(job.d_flag);

    // ---- 3. emit
    uint8_t *d_merged = nullptr;
    if ((e = arena.take(&d_merged, job.ntiles * kMergeTile)) != hipSuccess) return failed("the merged symbols");
    if ((e = state.tile_starts(d_cur)) != hipSuccess) return failed("emitting the merged symbols");
    state.emit(d_cur, d_merged);
    if ((e = hipGetLastError()) != hipSuccess || (e = lap(kMergeEmit)) != hipSuccess) return failed("emitting the merged symbols");
    arena.give_back(job.d_sym);
    arena.give_back(job.d_counts);

    // ---- 4. encode
    uint8_t *d_out = nullptr;
    uint64_t need = 0;
    if ((e = encode_symbol_runs(arena, d_merged, total, stream, &d_out, &need, &step)) != hipSuccess) return failed(step);
    if ((e = lap(kMergeEncode)) != hipSuccess) return failed("writing the runs");
    out->d_rle = arena.keep(d_out);
    out->rle_bytes = need;
    out->d_state = reinterpret_cast<uint8_t *>(arena.keep(d_cur));
    out->state_bytes = State::out_bytes(job);
    return hipSuccess;
}

}  // namespace

}  // namespace msbwt
