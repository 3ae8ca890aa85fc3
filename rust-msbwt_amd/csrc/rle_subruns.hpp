// The digit rule of the RLE byte stream (src/msbwt_core.rs:3-14 of the reference), byte by byte, for everything that does not
// walk whole runs on the host (that is rle_codec.hpp's for_each_run): byte = symbol | digit << 3, and every byte is a SUB-RUN of
// digit << 5 e symbols of its symbol, e = the consecutive bytes of that symbol right before it.  32^8 = 2^40 = kMaxSymbols, so a
// non-zero digit at e >= kMaxDigits alone makes the stream too large; such a byte counts as zero symbols and is flagged.
//
//   next_exponent, subrun_value, subrun_too_large
//                     the recurrence over the bytes, host and device: scan_merge_input (merge.hip) and the device walk
//   ThreadBytes, load_thread_bytes, for_each_subrun
//                     the device walk: a thread's 16 bytes, how their first byte continues a run that started before them, and
//                     fn(symbol, symbols) per byte.  device_build.hip (k_tile_sums, k_paint) and merge.hip's decoder
//                     (k_decode_sums, k_decode_paint) tile a stream with it, 256 threads x 16 bytes.
#pragma once
#include <cstdint>

#include "rle_codec.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSBWT_HOST_DEVICE __host__ __device__
#else
#define MSBWT_HOST_DEVICE
#endif

namespace msbwt {

constexpr int kMaxDigits = 8;               // digits a run of fewer than kMaxSymbols symbols can need
constexpr uint32_t kRleBadSymbol = 1u;      // error bit: a byte carries symbol code 6 or 7
constexpr uint32_t kRleTooLarge = 2u;       // error bit: a non-zero digit at e >= kMaxDigits
static_assert((1ull << (5 * kMaxDigits)) == kMaxSymbols, "the digit limit is the symbol limit");

// The recurrence over the bytes of a stream, host and device.  e: the bytes of the byte's symbol right before it, capped at
// kMaxDigits (from there on every byte is alike); signed, as the device compiler likes its shift counts.
MSBWT_HOST_DEVICE inline int next_exponent(int e, bool same_symbol) { return !same_symbol ? 0 : e < kMaxDigits ? e + 1 : kMaxDigits; }
// the symbols a byte stands for
MSBWT_HOST_DEVICE inline uint64_t subrun_value(uint32_t digit, int e) { return e < kMaxDigits ? uint64_t(digit) << (5 * e) : uint64_t(0); }
// a non-zero digit that cannot be
MSBWT_HOST_DEVICE inline bool subrun_too_large(uint32_t digit, int e) { return e >= kMaxDigits && digit != 0u; }

#if defined(__HIPCC__)
// The 16 bytes a thread owns and how their first byte continues a run that started earlier: `carry` = number of bytes right
// before them with the symbol of byte 0 (of the 16 before: more than kMaxDigits make no difference).  Three plain values, so
// that they stay in registers: four words picked by a byte's index, or two counters beside them, cost the loader's k_paint a
// copy in LDS or a wave of occupancy.
struct ThreadBytes {
    uint64_t lo, hi;  // bytes 0..7 and 8..15, the first the lowest
    uint32_t counts;  // how many of the 16 bytes exist | carry << 8
    __device__ __forceinline__ int valid() const { return int(counts & 0xFFu); }
    __device__ __forceinline__ int carry() const { return int(counts >> 8); }
};

// rle is 16-byte aligned and first is a multiple of 16; nothing at or past rle + n is read
__device__ __forceinline__ ThreadBytes load_thread_bytes(const uint8_t *__restrict__ rle, uint64_t n, uint64_t first) {
    const int valid = first >= n ? 0 : int(min(uint64_t(16), n - first));
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (valid == 16) {
        const uint4 c = *reinterpret_cast<const uint4 *>(rle + first);
        w0 = c.x; w1 = c.y; w2 = c.z; w3 = c.w;
    } else {
        for (int i = 0; i < valid; ++i) {
            const uint32_t b = uint32_t(rle[first + i]) << ((i & 3) * 8), word = uint32_t(i) >> 2;
            w0 |= word == 0u ? b : 0u;
            w1 |= word == 1u ? b : 0u;
            w2 |= word == 2u ? b : 0u;
            w3 |= word == 3u ? b : 0u;
        }
    }
    int carry = 0;
    if (first >= 16 && valid > 0) {
        const uint4 p = *reinterpret_cast<const uint4 *>(rle + first - 16);
        const uint32_t pw[4] = {p.x, p.y, p.z, p.w};
        const uint32_t sym0 = w0 & 7u;
        bool run = true;
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            run = run && (((pw[j >> 2] >> ((j & 3) * 8)) & 7u) == sym0);
            carry += run ? 1 : 0;
        }
    }
    return ThreadBytes{uint64_t(w1) << 32 | w0, uint64_t(w3) << 32 | w2, uint32_t(valid) | uint32_t(carry) << 8};
}

// Calls fn(sym, value) for each of the thread's sub-runs in order.  Returns error bits (kRleBadSymbol, kRleTooLarge).
template <class Fn>
__device__ __forceinline__ uint32_t for_each_subrun(const ThreadBytes &tb, Fn &&fn) {
    uint32_t bad = 0, prev_sym = 8;
    uint64_t lo = tb.lo, hi = tb.hi;  // the next byte is the lowest: the 16 shift down as one
    const int valid = tb.valid();
    int e = tb.carry();
    for (int i = 0; i < valid; ++i) {
        const uint32_t byte = uint32_t(lo) & 0xFFu, sym = byte & 7u, digit = byte >> 3;
        lo = (lo >> 8) | (hi << 56);
        hi >>= 8;
        if (i > 0) e = next_exponent(e, sym == prev_sym);
        prev_sym = sym;
        if (sym >= uint32_t(kAlphabet)) bad |= kRleBadSymbol;
        if (subrun_too_large(digit, e)) bad |= kRleTooLarge;
        fn(sym, subrun_value(digit, e));
    }
    return bad;
}
#endif

}  // namespace msbwt

#undef MSBWT_HOST_DEVICE
