// The source colouring of a loaded index: attaching and detaching the source vector, its size plan and its totals.  Calls
// source_index.hip through its header and handle.hpp; the by-source queries themselves are in query.cpp.
#include <algorithm>
#include <string>
#include <vector>

#include "handle.hpp"

namespace {

// bytes the attachment holds in HBM; MSBWT_ERR_* for arguments no attachment can have
int plan_bytes(uint64_t total_rows, size_t n_sources, uint64_t *bytes) {
    if (n_sources < 1 || n_sources > MSBWT_MERGE_MAX_INPUTS) return MSBWT_ERR_INVALID_ARG;
    if (total_rows >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    const SourceSizes z = source_sizes(total_rows, uint32_t(n_sources));
    *bytes = z.row_bytes + z.checkpoint_bytes;
    return MSBWT_OK;
}

}  // namespace

namespace msbwt_capi {

int attach_sources(msbwt_rle *h, const uint8_t *host_rows, const uint8_t *device_rows, uint64_t n_rows, size_t n_sources) {
    h->sources.release();
    uint64_t bytes = 0;
    if (n_rows != h->totals.total) return fail(h, MSBWT_ERR_INVALID_ARG, "the source vector has " + std::to_string(n_rows) + " rows, the index " + std::to_string(h->totals.total));
    if (plan_bytes(n_rows, n_sources, &bytes)) return fail(h, MSBWT_ERR_INVALID_ARG, "sources: 1 <= n_sources <= " + std::to_string(MSBWT_MERGE_MAX_INPUTS));
    if (n_rows && !host_rows && !device_rows) return fail(h, MSBWT_ERR_INVALID_ARG, "sources must not be null with rows");
    if (int rc = ensure_runtime(h)) return rc;
    const SourceSizes z = source_sizes(n_rows, uint32_t(n_sources));
    const std::string need = "source index: " + std::to_string(bytes) + " bytes of HBM needed, and " + std::to_string(z.scratch_bytes) + " more while it is built";
    size_t free_bytes = 0, all_bytes = 0;
    HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
    if (free_bytes < bytes + z.scratch_bytes) return fail(h, MSBWT_ERR_HIP, need);
    SourceIndex made;
    void *scratch = nullptr;
    auto give_up = [&](int rc) {
        made.release();
        if (scratch) (void)hipFree(scratch);
        return rc;
    };
    if ((z.row_bytes && hipMalloc(&made.rows, z.row_bytes) != hipSuccess) || hipMalloc(&made.checkpoints, z.checkpoint_bytes) != hipSuccess ||
        hipMalloc(&scratch, z.scratch_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(fail(h, MSBWT_ERR_HIP, need));
    }
    uint8_t *rows = static_cast<uint8_t *>(made.rows);
    hipError_t e = hipSuccess;
    if (device_rows && n_rows) {
        e = hipMemcpyAsync(rows, device_rows, n_rows, hipMemcpyDeviceToDevice, h->stream);
    } else if (n_rows) {  // in pieces of 16 MiB through the pinned staging of the host batches: no second host copy of the vector
        e = h->pipe.run(n_rows, size_t(1) << 24, {HostArray{host_rows, nullptr, 1}}, {}, h->stream,
                        [&](size_t first, size_t m, void *const *d_in, void *const *, hipStream_t stream) {
                            return hipMemcpyAsync(rows + first, d_in[0], m, hipMemcpyDeviceToDevice, stream);
                        });
    }
    if (e != hipSuccess) return give_up(hip_fail(h, e, "source vector upload"));
    uint32_t *d_bad = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(h->d_flags) + kSourceBadOffset);
    uint32_t bad = 0;
    const uint32_t stride = source_stride(uint32_t(n_sources));
    e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = launch_source_build(rows, n_rows, uint32_t(n_sources), static_cast<uint64_t *>(made.checkpoints), static_cast<uint64_t *>(scratch), d_bad, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)  // the last checkpoint: the totals
        e = hipMemcpyAsync(made.totals, static_cast<uint64_t *>(made.checkpoints) + z.nblocks * stride, n_sources * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return give_up(hip_fail(h, e, "source index build"));
    if (bad) return give_up(fail(h, MSBWT_ERR_INVALID_ARG, "the source vector holds a byte >= n_sources (" + std::to_string(n_sources) + ")"));
    (void)hipFree(scratch);
    made.n_sources = uint32_t(n_sources);
    made.bytes = bytes;
    h->sources = made;
    h->err.clear();
    return MSBWT_OK;
}

}  // namespace msbwt_capi

extern "C" {

int msbwt_rle_set_sources(msbwt_rle *bwt, const uint8_t *sources, uint64_t n_rows, size_t n_sources) {
    Call c(bwt);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (!sources && n_sources == 0) {  // detach
        if (int rc = c.bind()) return rc;
        h->sources.release();
        return MSBWT_OK;
    }
    if (int rc = c.open()) return rc;
    return attach_sources(h, sources, nullptr, n_rows, n_sources);
}

int msbwt_rle_source_count(const msbwt_rle *bwt) { return bwt ? int(bwt->sources.n_sources) : 0; }

int msbwt_rle_source_totals(const msbwt_rle *bwt, uint64_t *out) {
    Call c(bwt);
    if (!c.h || !out) return MSBWT_ERR_INVALID_ARG;
    if (int rc = c.loaded()) return rc;
    const SourceIndex &s = c.h->sources;
    if (!s.n_sources) return fail(c.h, MSBWT_ERR_NOT_LOADED, "no sources attached");
    std::copy(s.totals, s.totals + s.n_sources, out);
    return MSBWT_OK;
}

int msbwt_source_index_plan(uint64_t total_rows, size_t n_sources, uint64_t *device_bytes) {
    uint64_t bytes = 0;
    if (int rc = plan_bytes(total_rows, n_sources, &bytes)) return rc;
    if (device_bytes) *device_bytes = bytes;
    return MSBWT_OK;
}

size_t msbwt_source_block_rows(void) { return kSourceBlockRows; }

size_t msbwt_source_narrow_rows(void) { return kSourceNarrow; }

}  // extern "C"
