// gfx950: the two streaming passes of the canonical k-mer calls (canonical.hpp) over the k-mers a chunk of the walk staged: the reverse
// complements as packed words for the search, and -- with the search's counts -- the classes.
//
// Which member emits.  A class {q, rc(q)} with counts c and c' is emitted by q iff c > c', or c == c' and q <= rc(q): by exactly one of
// its members when both are staged, and by the only one there when the other is absent from the index or was pruned away.  With a
// window minimum m the walk prunes at ceil(m / 2): of two counts that sum to m or more the larger is at least ceil(m / 2), and so is every
// suffix of that member, so the emitting member always reaches the last level.  (The canonical member as the emitter would be lost
// whenever it is the rarer strand; pruning at m loses a class seen once on each strand at m = 2.)  A palindrome is its own reverse
// complement: c' == c, it emits itself as (q, c, 0).
// One thread per staged k-mer: 24 + 16 bytes in, at most 24 out; integer work, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "canonical.hpp"
#include "frontier.hpp"
#include "kernels.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = kFrontierThreads;
constexpr uint32_t kLdsBins = 2048;  // class counts below this are tallied in LDS (8 KB), as in the spectrum's histogram sink

uint32_t grid_for(uint64_t m) { return capped_grid(m, kThreads, 256u * 8u); }

__global__ __launch_bounds__(kThreads) void k_canonical_rc(const Node *__restrict__ staged, uint64_t m, uint32_t k, uint64_t *__restrict__ rc_words) {
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < m; i += uint64_t(gridDim.x) * kThreads) rc_words[i] = reverse_complement_2bit(staged[i].key, k);
}

__global__ __launch_bounds__(kThreads) void k_canonical_combine(const Node *__restrict__ staged, const uint64_t *__restrict__ rc_words, const uint64_t *__restrict__ rc_counts,
                                                               uint64_t m, CanonicalSink sink) {
    __shared__ uint32_t lds_hist[kLdsBins];
    const bool hist = sink.mode == kCanonicalHist;
    if (hist) {
        for (uint32_t b = threadIdx.x; b < kLdsBins; b += kThreads) lds_hist[b] = 0u;
        __syncthreads();
    }
    uint64_t occurrences = 0;
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < m; base += uint64_t(gridDim.x) * kThreads) {  // (the same trips for the whole workgroup)
        const uint64_t i = base + threadIdx.x;
        uint64_t w = 0, own = 0, other = 0;
        bool emit = false;
        if (i < m) {
            const Node nd = staged[i];
            const uint64_t q = nd.key, c = nd.h - nd.l, r = rc_words[i], c2 = rc_counts[i];
            const bool canonical = q <= r;
            w = canonical ? q : r;
            own = canonical ? c : c2;
            other = canonical ? (q == r ? 0ull : c2) : c;
            const uint64_t count = own + other;
            emit = (c > c2 || (c == c2 && canonical)) && count >= sink.min && count <= sink.max;
        }
        block_add(emit ? 1u : 0u, sink.totals + kCanonicalClasses);
        if (hist) {
            if (emit) {
                const uint64_t count = own + other, bin = min(count, sink.n_bins - 1u);
                if (bin < kLdsBins) atomicAdd(&lds_hist[bin], 1u);
                else atomicAdd(sink.hist + bin, 1ull);
                occurrences += count;
            }
        } else if (sink.mode == kCanonicalAppend) {
            const uint64_t at = reserve(emit ? 1u : 0u, sink.totals + kCanonicalOut);
            if (emit) {
                if (at < sink.capacity) {
                    sink.kmers[at] = w;
                    if (sink.own) sink.own[at] = own;
                    if (sink.other) sink.other[at] = other;
                } else {
                    atomicOr(sink.flags, kFlagInternal);
                }
            }
        }
    }
    if (hist) {
        __syncthreads();
        const uint32_t bins = uint32_t(min(uint64_t(kLdsBins), sink.n_bins));
        for (uint32_t b = threadIdx.x; b < bins; b += kThreads) {
            const uint32_t c = lds_hist[b];
            if (c) atomicAdd(sink.hist + b, (unsigned long long)c);
        }
        const unsigned long long s = wave_sum<unsigned long long>(occurrences);  // one atomic per wave
        if ((threadIdx.x & 63u) == 0u && s) atomicAdd(sink.totals + kCanonicalOccurrences, s);
    }
}

}  // namespace

hipError_t launch_canonical_rc(const void *d_staged, uint64_t m, uint32_t k, uint64_t *rc_words, hipStream_t stream) {
    if (!d_staged || !rc_words || k < 1 || k > 32) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_canonical_rc, dim3(grid_for(m)), dim3(kThreads), 0, stream, static_cast<const Node *>(d_staged), m, k, rc_words);
    return hipGetLastError();
}

hipError_t launch_canonical_combine(const void *d_staged, const uint64_t *rc_words, const uint64_t *rc_counts, uint64_t m, const CanonicalSink &sink, hipStream_t stream) {
    const bool ok = sink.mode == kCanonicalHist ? (sink.hist && sink.n_bins >= 2) : sink.mode == kCanonicalAppend ? (sink.kmers && sink.flags) : sink.mode == kCanonicalCount;
    if (!d_staged || !rc_words || !rc_counts || !sink.totals || !ok) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_canonical_combine, dim3(grid_for(m)), dim3(kThreads), 0, stream, static_cast<const Node *>(d_staged), rc_words, rc_counts, m, sink);
    return hipGetLastError();
}

}  // namespace msbwt
