// A byte per slot, four slots a 32-bit word: the edge bytes of the k-mer graph (kmer_graph.hpp) and the link bytes of the unitigs
// (unitigs.hpp).  Neighbouring slots belong to other threads, so bits are set and cleared by vector atomics on the word.
// Include from HIP translation units only (the names are per translation unit, as in workgroup.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace msbwt {
namespace {

__device__ __forceinline__ uint32_t byte_of(const uint32_t *__restrict__ words, uint64_t slot) { return (words[slot >> 2] >> (8u * (uint32_t(slot) & 3u))) & 0xFFu; }
__device__ __forceinline__ void or_slot_bits(uint32_t *__restrict__ words, uint64_t slot, uint32_t bits) { atomicOr(words + (slot >> 2), bits << (8u * (uint32_t(slot) & 3u))); }
__device__ __forceinline__ void clear_slot_bits(uint32_t *__restrict__ words, uint64_t slot, uint32_t bits) { atomicAnd(words + (slot >> 2), ~(bits << (8u * (uint32_t(slot) & 3u)))); }

}  // namespace
}  // namespace msbwt
