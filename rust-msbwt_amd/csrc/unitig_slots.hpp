// WORD -> SLOT and SLOT -> HEAD over the arrays both unitig calls hold behind the ranking (unitigs.hpp): what the link kernels
// (unitig_links.hip) and the by-source sums (unitig_sources.hip) both ask of a slot.
// Include from HIP translation units only (the names are per translation unit, as in slot_bytes.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "unitigs.hpp"

namespace msbwt {
namespace {

// the slot of w among the n sorted words, or n where w is none of them; `probes` halvings at the most
__device__ __forceinline__ uint64_t slot_of(const uint64_t *__restrict__ words, uint64_t n, uint32_t probes, uint64_t w) {
    uint64_t lo = 0, hi = n;
    for (uint32_t step = 0; step < probes && lo < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (words[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && words[lo] == w ? lo : n;
}

// the head of slot i's unitig, or n where the ranking left none (the host ranks until nothing is unfinished)
__device__ __forceinline__ uint64_t head_of(const UnitigNodes &g, const UnitigState *__restrict__ state, uint64_t i) {
    const UnitigState s = state[i];
    return (s.y & kUnitigDone) && s.x < g.n ? uint64_t(s.x) : g.n;
}

}  // namespace
}  // namespace msbwt
