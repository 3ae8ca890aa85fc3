// Canonical k-mers (canonical.hip; msbwt_rle_canonical_kmer_spectrum, msbwt_rle_enumerate_canonical_kmers[_device]): a k-mer q and its
// reverse complement rc(q) are ONE class, named by the smaller of their packed 2-bit words w (word order is lexicographic order) and
// reported once as (w, own = count_kmer(w), other = count_kmer(rc(w))); a palindrome (w == rc(w), even k only) has other = 0.  The
// class count is own + other.
// How: the walk of spectrum.hip stages a chunk's k-mers (spectrum_stage), launch_canonical_rc writes their reverse complements as
// packed words, the library's packed search (launch_count_2bit) counts those, and launch_canonical_combine emits every class from
// exactly one of its members -- the one that occurs more often, on a tie the canonical one -- so that a class is found whichever of
// its two strands the index holds and whichever the walk's pruning let through.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace msbwt {

// packed reverse complement of a k-mer, 1 <= k <= 32: the k 2-bit fields in reverse order, each XOR 3
#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
inline uint64_t reverse_complement_2bit(uint64_t w, uint32_t k) {
    w = ((w >> 2) & 0x3333333333333333ull) | ((w & 0x3333333333333333ull) << 2);
    w = ((w >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((w & 0x0F0F0F0F0F0F0F0Full) << 4);
    w = ((w >> 8) & 0x00FF00FF00FF00FFull) | ((w & 0x00FF00FF00FF00FFull) << 8);
    w = ((w >> 16) & 0x0000FFFF0000FFFFull) | ((w & 0x0000FFFF0000FFFFull) << 16);
    w = (w >> 32) | (w << 32);
    return ~w >> (64u - 2u * k);
}

constexpr int kCanonicalHist = 0, kCanonicalCount = 1, kCanonicalAppend = 2;
constexpr int kCanonicalClasses = 0, kCanonicalOccurrences = 1, kCanonicalOut = 2, kCanonicalTotalWords = 4;  // words of CanonicalSink::totals
constexpr uint64_t kCanonicalStageBytes = 2 * sizeof(uint64_t);  // per frontier node: the other strand's word and its count

struct CanonicalSink {
    int mode;
    uint64_t min, max;           // the window of the class count (max: all-ones = none)
    unsigned long long *hist;    // kCanonicalHist: hist[min(count, n_bins - 1)] += 1
    uint64_t n_bins;
    uint64_t *kmers, *own, *other;  // kCanonicalAppend (own, other optional); nothing is written at or beyond capacity (*flags |= kFlagInternal)
    uint64_t capacity;
    uint32_t *flags;
    unsigned long long *totals;  // kCanonicalTotalWords words, zeroed by the caller: classes in the window, the sum of their counts (histogram), records appended
};

// rc_words[i] = reverse complement of the staged k-mer i (d_staged: the m records {word, l, h} spectrum_stage hands over)
hipError_t launch_canonical_rc(const void *d_staged, uint64_t m, uint32_t k, uint64_t *rc_words, hipStream_t stream);
// staged k-mer i occurs h - l times and its reverse complement rc_words[i] rc_counts[i] times: the classes these m members emit go to the sink
hipError_t launch_canonical_combine(const void *d_staged, const uint64_t *rc_words, const uint64_t *rc_counts, uint64_t m, const CanonicalSink &sink, hipStream_t stream);

}  // namespace msbwt
