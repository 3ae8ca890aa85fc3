// What the device builders share (run_encode.hip): the exclusive scan of u64 in HBM, the arena of a build's allocations, and the
// encoder symbols -> RLE bytes.  reads_build.hip and merge.hip both call this one copy.  The primitives inside a workgroup
// (prefix sum, wave sums, ceil_div, capped_grid) are workgroup.hpp's; this header is for host translation units as well.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

namespace msbwt {

constexpr uint32_t kScanThreads = 256, kScanWaves = kScanThreads / 64;  // every kernel of the builders runs 256 threads

// words of scratch a scan of n elements needs (the sums of every level)
uint64_t scan_scratch_words(uint64_t n);
// exclusive scan of d[0 .. n), in place
hipError_t exclusive_scan(uint64_t *d, uint64_t n, uint64_t *scratch, hipStream_t stream);

// device allocations of one build: whatever is still held when the build ends, however it ends, is freed
struct Arena {
    std::vector<void *> held;
    uint64_t taken = 0;  // bytes of every allocation made through take(), given back or not: what a call's scratch came to
    ~Arena() {
        for (void *p : held) (void)hipFree(p);
    }
    template <class T>
    hipError_t take(T **p, uint64_t bytes) {
        void *raw = nullptr;
        const hipError_t e = hipMalloc(&raw, size_t(std::max<uint64_t>(bytes, 256)));
        if (e == hipSuccess) {
            held.push_back(raw);
            taken += std::max<uint64_t>(bytes, 256);
        }
        *p = static_cast<T *>(raw);
        return e;
    }
    template <class T>
    void give_back(T *&p) {
        held.erase(std::remove(held.begin(), held.end(), static_cast<void *>(p)), held.end());
        (void)hipFree(p);
        p = nullptr;
    }
    template <class T>
    T *keep(T *p) {  // the caller owns it from here on
        held.erase(std::remove(held.begin(), held.end(), static_cast<void *>(p)), held.end());
        return p;
    }
};

// symbols[0 .. total) in HBM, total >= 1 -> their RLE bytes (src/msbwt_core.rs:3-14, the canonical encoding convert_to_vec gives)
// in an allocation of the arena: *d_rle, *rle_bytes.  The stream is drained when it returns.  On failure *what names the step.
hipError_t encode_symbol_runs(Arena &arena, const uint8_t *d_symbols, uint64_t total, hipStream_t stream, uint8_t **d_rle, uint64_t *rle_bytes,
                              const char **what);

}  // namespace msbwt
