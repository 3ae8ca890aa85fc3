// The query path: batch order, the launches behind every count / range / extension entry point, their host pipelines and the mailbox
// of the small host batches.  Calls the kernels' host launchers and handle.hpp; nothing here builds or frees a part of the index.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "gather.hpp"
#include "handle.hpp"
#include "order.hpp"

namespace {

// mailbox layout (bytes); kMailQueries queries of at most kMailKmerBytes in all
constexpr size_t kMailQueries = 64, kMailKmerBytes = 4096;
constexpr size_t kMailDone = 0;  // u64 completion word (lanes kernel, one wave)
constexpr size_t kMailKmers = 64, kMailCounts = kMailKmers + kMailKmerBytes, kMailSyms = kMailCounts + 8 * kMailQueries,
                 kMailL = kMailSyms + 64, kMailH = kMailL + 8 * kMailQueries, kMailOutL = kMailH + 8 * kMailQueries,
                 kMailOutH = kMailOutL + 8 * kMailQueries, kMailBytes = kMailOutH + 8 * kMailQueries;

int ensure_mail(msbwt_rle *h) {  // (and the handle's stream and status block: ensure_runtime)
    if (int rc = ensure_runtime(h)) return rc;
    if (h->mail) return MSBWT_OK;
    void *host = nullptr, *dev = nullptr;
    // coherent explicitly: the host polls a word the kernel writes (HIP_HOST_COHERENT=0 in the environment must not turn every
    // single-query call into a 2 ms spin)
    HIP_TRY(h, hipHostMalloc(&host, kMailBytes, hipHostMallocMapped | hipHostMallocCoherent));
    const hipError_t e = hipHostGetDevicePointer(&dev, host, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(host);
        return hip_fail(h, e, "hipHostGetDevicePointer");
    }
    std::memset(host, 0, kMailBytes);
    h->mail = static_cast<uint8_t *>(host);
    h->d_mail = static_cast<uint8_t *>(dev);
    return MSBWT_OK;
}

// Batch order (order.hip): is this launch to be put through the ordering passes?  Mode 1: whenever they apply (lanes kernel
// on a pair index, 12 <= k <= 64, 4096 <= n < 2^32).  Automatic (-1, the default) is NEVER, on the measurements of round 4
// (profiles/r04_lab/library_batch_order.log, one box, pass off / on): 10^8 read-derived 31-mers over the C4 index 16.8 ->
// 16.1 ms, with repeats 18.9 -> 18.7, C3 3.13 -> 2.97 -- a few per cent where the batch is dense -- against 3.4 -> 9.3 ms on
// random 31-mers (which end in the table: nothing to order for), 5.5 -> 6.6 on 3 x 10^7 queries and 55.7 -> 79.9 at human
// scale.  The ordered search itself is worth 2x (8.4 ms when the caller hands the batch over sorted, msbwt_kmer_order_keys),
// but packing, two bucket passes and returning the counts to the caller's order cost 6 ms of it for 10^8 queries, and the
// search pays 1.7 ms more for a 22-bit order and placed count stores.  Nothing a launch knows beforehand tells the first
// case from the others by a margin that would justify the risk, so the pass stays a switch.
bool order_pays(msbwt_rle *h, const IndexView &v, size_t k, size_t n) {
    if (h->wanted_order <= 0 || v.block_format != kBlocksPlanes || v.pair_blocks == nullptr) return false;
    return k >= 12 && k <= 64 && n >= 4096 && n <= 0xFFFFFFFFull && lanes_serves(v, uint32_t(k));
}

// grows the slot's ordering scratch; false = no memory for it (the launch then runs unordered)
bool ensure_order_scratch(msbwt_rle::TicketSlot &slot, size_t bytes) {
    if (bytes <= slot.order_bytes) return true;
    if (slot.order_scratch) (void)hipFree(slot.order_scratch);  // (waits for the device: nothing still reads it)
    slot.order_scratch = nullptr;
    slot.order_bytes = 0;
    if (hipMalloc(&slot.order_scratch, bytes) != hipSuccess) {
        (void)hipGetLastError();
        slot.order_scratch = nullptr;
        return false;
    }
    slot.order_bytes = bytes;
    return true;
}

uint32_t order_reach(const IndexView &v, size_t k) {  // the symbols the bucket key reads: the table's own index, else 17
    const uint32_t depth = (v.table.entries && v.table.depth > 0 && size_t(v.table.depth) <= k) ? uint32_t(v.table.depth) : 17u;
    return uint32_t(std::min<size_t>(depth, k));
}

// The batch through the ordering passes (order.hip) when they pay and have scratch: rows (d_kmers, then the exceptions pass) or 2-bit
// words (d_packed).  false = not ordered, nothing enqueued.
bool launch_ordered(msbwt_rle *h, const IndexView &v, msbwt_rle::TicketSlot &slot, const uint8_t *d_kmers, const uint64_t *d_packed, size_t k, size_t n,
                    uint64_t *d_out, hipStream_t stream, int which, hipError_t *e) {
    if (!order_pays(h, v, k, n)) return false;
    const OrderPlan plan = plan_order(n, uint32_t(k), order_reach(v, k), uint32_t(h->order_bits), d_kmers != nullptr);
    if (!ensure_order_scratch(slot, plan.scratch_bytes)) return false;
    const uint64_t *ordered = nullptr;
    bool inline_place = false;
    uint64_t *counts = nullptr;
    *e = launch_order_batch(plan, d_kmers, d_packed, slot.order_scratch, stream, &ordered, &inline_place, &counts);
    if (*e == hipSuccess) *e = launch_count_packed(v, ordered, uint32_t(k), n, counts, nullptr, h->d_flags + which, stream, plan.words + 1, inline_place);
    if (*e == hipSuccess) *e = launch_order_finish(plan, slot.order_scratch, d_out, stream);
    if (*e == hipSuccess && d_kmers) *e = launch_count_exceptions(plan, v.blocks, v.total, d_kmers, slot.order_scratch, d_out, h->d_flags + which, stream);
    return true;
}

}  // namespace

namespace msbwt_capi {

int launch_count(msbwt_rle *h, const uint8_t *d_kmers, size_t k, size_t n, uint64_t *d_out, hipStream_t stream, int which) {
    if (k > 0xFFFFFFFFull) return fail(h, MSBWT_ERR_INVALID_ARG, "k does not fit 32 bits");
    return timed_launch(h, stream, [&] {
        return with_slot(h, stream, [&](const IndexView &v, msbwt_rle::TicketSlot &slot) {
            hipError_t e = hipSuccess;
            if (launch_ordered(h, v, slot, d_kmers, nullptr, k, n, d_out, stream, which, &e)) return e;
            return launch_count_kmers(v, d_kmers, uint32_t(k), n, d_out, h->d_flags + which, stream);
        });
    });
}

// the same for queries handed over as 2-bit words (include/msbwt_hip.h, msbwt_rle_count_kmers_packed_device; the canonical walk of walk_call.cpp, the canonical unitigs and the traces)
int launch_count_2bit(msbwt_rle *h, const uint64_t *d_packed, size_t k, size_t n, uint64_t *d_out, hipStream_t stream, int which) {
    if (k < 1 || k > 64) return fail(h, MSBWT_ERR_INVALID_ARG, "packed queries need 1 <= k <= 64");
    if (reinterpret_cast<uintptr_t>(d_packed) & 7u) return fail(h, MSBWT_ERR_INVALID_ARG, "packed queries must be 8-byte aligned");
    return timed_launch(h, stream, [&] {
        return with_slot(h, stream, [&](const IndexView &v, msbwt_rle::TicketSlot &slot) {
            if (v.block_format != kBlocksPlanes) {  // run blocks: no kernel reads 2-bit words; unpack into rows first
                const size_t row_bytes = (n * k + 255) / 256 * 256;
                if (!ensure_order_scratch(slot, row_bytes)) return hipErrorOutOfMemory;
                uint8_t *rows = static_cast<uint8_t *>(slot.order_scratch);
                hipError_t e = launch_unpack_rows(d_packed, uint32_t(k), n, rows, stream);
                if (e == hipSuccess) e = launch_count_kmers(v, rows, uint32_t(k), n, d_out, h->d_flags + which, stream);
                return e;
            }
            hipError_t e = hipSuccess;
            if (launch_ordered(h, v, slot, nullptr, d_packed, k, n, d_out, stream, which, &e)) return e;
            return launch_count_packed(v, d_packed, uint32_t(k), n, d_out, nullptr, h->d_flags + which, stream);
        });
    });
}

}  // namespace msbwt_capi

namespace {

// FM ranges of n k-mers (msbwt_rle_kmer_ranges[_device]): l to d_l[i * stride], h to d_h[i * stride].  Never ordered: the search
// runs in the caller's order, in the kRange form of the kernel launch_count would pick (launch_kmer_ranges).
int launch_ranges(msbwt_rle *h, const uint8_t *d_kmers, size_t k, size_t n, uint64_t *d_l, uint64_t *d_h, uint32_t stride, hipStream_t stream,
                  int which) {
    if (k > 0xFFFFFFFFull) return fail(h, MSBWT_ERR_INVALID_ARG, "k does not fit 32 bits");
    return timed_with_tickets(h, stream, [&](const IndexView &v) {
        return launch_kmer_ranges(v, d_kmers, uint32_t(k), n, d_l, d_h, stride, h->d_flags + which, stream);
    });
}

// Left-extension counts (msbwt_rle_count_kmer_extensions[_device]) in two launches and no scratch: the range of row i goes into the
// first 16 bytes of its own 48-byte output row, and extend.hip turns the row into the six counts in place.
int launch_extensions(msbwt_rle *h, const uint8_t *d_kmers, size_t k, size_t n, uint64_t *d_out, hipStream_t stream, int which) {
    if (k > 0xFFFFFFFFull) return fail(h, MSBWT_ERR_INVALID_ARG, "k does not fit 32 bits");
    return timed_with_tickets(h, stream, [&](const IndexView &v) {
        hipError_t e = launch_kmer_ranges(v, d_kmers, uint32_t(k), n, d_out, d_out + 1, 6u, h->d_flags + which, stream);
        if (e == hipSuccess) e = launch_kmer_extensions(v, d_out, n, h->d_flags + which, stream);
        return e;
    });
}

// grows the slot's scratch of range pairs; false = no memory for it
bool ensure_range_scratch(msbwt_rle::TicketSlot &slot, size_t bytes) {
    if (bytes <= slot.range_bytes) return true;
    if (slot.range_scratch) (void)hipFree(slot.range_scratch);  // (waits for the device: nothing still reads it)
    slot.range_scratch = nullptr;
    slot.range_bytes = 0;
    if (hipMalloc(&slot.range_scratch, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    slot.range_bytes = bytes;
    return true;
}

constexpr size_t kBySourcePiece = size_t(1) << 23;  // queries whose ranges the scratch holds at once (128 MiB: they stay in the Infinity Cache between the phases)

// Counts by source (msbwt_rle_count_kmers_by_source[_device]) in two launches per piece: the ranges go as dense {l, h} pairs into the slot's
// scratch -- not into the output rows, which are 8 bytes with one source and strided stores otherwise -- and source_index.hip turns them
// into the rows.  The scratch grows to the largest piece seen and stays: no allocation in the steady state.
int launch_by_source(msbwt_rle *h, const uint8_t *d_kmers, size_t k, size_t n, uint64_t *d_out, hipStream_t stream, int which) {
    if (k > 0xFFFFFFFFull) return fail(h, MSBWT_ERR_INVALID_ARG, "k does not fit 32 bits");
    return timed_launch(h, stream, [&] {
        return with_slot(h, stream, [&](const IndexView &v, msbwt_rle::TicketSlot &slot) {
            if (!ensure_range_scratch(slot, std::min(n, kBySourcePiece) * 2 * sizeof(uint64_t))) return hipErrorOutOfMemory;
            uint64_t *pairs = static_cast<uint64_t *>(slot.range_scratch);
            const SourceView sv = h->sources.view(v.total);
            hipError_t e = hipSuccess;
            for (size_t first = 0; first < n && e == hipSuccess; first += kBySourcePiece) {
                const size_t m = std::min(kBySourcePiece, n - first);
                e = launch_kmer_ranges(v, d_kmers + first * k, uint32_t(k), m, pairs, pairs + 1, 2u, h->d_flags + which, stream);
                if (e == hipSuccess) e = launch_range_sources(sv, pairs, pairs + 1, 2u, m, d_out + first * sv.n_sources, h->d_flags + which, stream);
            }
            return e;
        });
    });
}

int launch_sources_of_ranges(msbwt_rle *h, const uint64_t *d_l, const uint64_t *d_h, size_t n, uint64_t *d_out, hipStream_t stream, int which) {
    return timed_launch(h, stream, [&] { return launch_range_sources(h->sources.view(h->totals.total), d_l, d_h, 1u, n, d_out, h->d_flags + which, stream); });
}

int need_sources(msbwt_rle *h) { return h->sources.n_sources ? int(MSBWT_OK) : fail(h, MSBWT_ERR_NOT_LOADED, "no sources attached"); }

// queries of a host batch's chunk when a result row holds one u64 per source: 2 Mi as the other batches, fewer once a row passes the extensions' 48 bytes
size_t by_source_chunk(const msbwt_rle *h) { return std::min(size_t(1) << 21, (size_t(96) << 20) / (h->sources.n_sources * sizeof(uint64_t))); }

// Enqueues the fused read -> k-mer count kernel; the caller holds h->mu and has made the
// handle's device current.
int launch_read_kmers_locked(msbwt_rle *h, const void *d_reads, size_t read_len, size_t n_reads, size_t k,
                                    int ascii, void *d_out_fwd, void *d_out_rc, hipStream_t stream, int which) {
    return timed_with_tickets(h, stream, [&](const IndexView &v) {
        return launch_count_read_kmers(v, static_cast<const uint8_t *>(d_reads), uint32_t(read_len), n_reads, uint32_t(k), ascii != 0,
                                       static_cast<uint64_t *>(d_out_fwd), static_cast<uint64_t *>(d_out_rc), h->d_flags + which, stream);
    });
}

HostArray host_in(const void *p, size_t item_bytes) { return HostArray{p, nullptr, item_bytes}; }
HostArray host_out(void *p, size_t item_bytes) { return HostArray{nullptr, p, item_bytes}; }

// A host-pointer batch through the pinned pipeline (host_pipeline.hpp): `launch` enqueues a chunk of m items; the batch's flags at the end.
template <class Launch>
int run_host_batch(msbwt_rle *h, size_t n, size_t chunk, const std::vector<HostArray> &ins, const std::vector<HostArray> &outs, const char *what,
                   Launch &&launch) {
    int launch_rc = MSBWT_OK;
    const hipError_t e = h->pipe.run(n, chunk, ins, outs, h->stream, [&](size_t, size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
        launch_rc = launch(m, d_in, d_out, stream);
        return launch_rc ? hipErrorUnknown : hipSuccess;
    });
    if (launch_rc) return launch_rc;
    if (e != hipSuccess) return hip_fail(h, e, (std::string(what) + " pipeline").c_str());
    return status_of(h, h->stream, kHostFlags);
}

// A small host batch through the mailbox (ensure_mail), its queries already there.  With `poll` the host polls the word the kernel writes
// on completion (v.done: ~5 us cheaper than a stream synchronisation; bounded: a kernel that never reports, a fault, is left to the
// synchronisation, which says why).  copy_out() says whether a result is the error sentinel u64::MAX: only then is the status word read.
template <class Launch, class CopyOut>
int mailbox_call(msbwt_rle *h, IndexView &v, bool poll, Launch &&launch, CopyOut &&copy_out) {
    volatile uint64_t *done = reinterpret_cast<volatile uint64_t *>(h->mail + kMailDone);
    const uint64_t seq = ++h->mail_seq;
    if (poll) {
        v.done = reinterpret_cast<uint64_t *>(h->d_mail + kMailDone);
        v.done_seq = seq;
    }
    if (int rc = launch()) return rc;
    bool seen = false;
    if (poll) {
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        for (unsigned spins = 0; !(seen = *done == seq); ++spins)
            if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() > give_up) break;
    }
    if (!seen) HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::atomic_thread_fence(std::memory_order_acquire);  // the results are read after the completion word
    return copy_out() ? status_of(h, h->stream, kHostFlags) : MSBWT_OK;
}

}  // namespace

extern "C" {

int msbwt_rle_count_kmers_device(const msbwt_rle *ch, const void *d_kmers, size_t k, size_t n,
                                 void *d_out_counts, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open(n && (!d_out_counts || (!d_kmers && k)), "null device pointer")) return rc;
    return launch_count(c.h, static_cast<const uint8_t *>(d_kmers), k, n, static_cast<uint64_t *>(d_out_counts),
                        static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

int msbwt_rle_count_kmers_packed_device(const msbwt_rle *ch, const void *d_kmers2bit, size_t k, size_t n, void *d_out_counts, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open(n && (!d_out_counts || !d_kmers2bit), "null device pointer")) return rc;
    if (n == 0) return MSBWT_OK;
    return launch_count_2bit(c.h, static_cast<const uint64_t *>(d_kmers2bit), k, n, static_cast<uint64_t *>(d_out_counts), static_cast<hipStream_t>(hip_stream),
                             kDeviceFlags);
}

int msbwt_rle_count_kmers_packed(const msbwt_rle *ch, const uint64_t *kmers2bit, size_t k, size_t n, void *out_counts, int count_bits) {
    Call c(ch);
    const bool bad_k = k < 1 || k > 64 || (count_bits != 64 && count_bits != 32);
    if (int rc = c.open(bad_k || (n && (!out_counts || !kmers2bit)), bad_k ? "packed queries need 1 <= k <= 64 and 64- or 32-bit counts" : "null pointer")) return rc;
    if (n == 0) return MSBWT_OK;
    msbwt_rle *h = c.h;
    if (int rc = ensure_runtime(h)) return rc;
    // pipelined like msbwt_rle_count_kmers: 8 (16) bytes per query in, 8 or 4 out; the 32-bit form counts into a device
    // buffer and narrows on the kernels' stream (a count beyond 32 bits is reported, not truncated silently)
    const size_t words = k > 32 ? 2 : 1, chunk = size_t(1) << 22;
    if (int rc = count_bits == 32 ? ensure_stage(h, std::min(n, chunk) * sizeof(uint64_t)) : MSBWT_OK) return rc;
    return run_host_batch(h, n, chunk, {host_in(kmers2bit, words * sizeof(uint64_t))}, {host_out(out_counts, size_t(count_bits / 8))}, "count_kmers_packed",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              uint64_t *d_counts = count_bits == 64 ? static_cast<uint64_t *>(d_out[0]) : static_cast<uint64_t *>(h->d_stage);
                              if (int r = launch_count_2bit(h, static_cast<const uint64_t *>(d_in[0]), k, m, d_counts, stream, kHostFlags)) return r;
                              if (count_bits == 64) return int(MSBWT_OK);
                              const hipError_t e = launch_narrow_counts32(d_counts, static_cast<uint32_t *>(d_out[0]), m, h->d_flags + kHostFlags, stream);
                              return e == hipSuccess ? int(MSBWT_OK) : hip_fail(h, e, "count_kmers_packed pipeline");
                          });
}

int msbwt_kmers_pack_2bit(const uint8_t *kmers, size_t k, size_t n, uint64_t *out_words) {
    if (k < 1 || k > 64 || (n && (!kmers || !out_words))) return MSBWT_ERR_INVALID_ARG;
    const size_t words = k > 32 ? 2 : 1;
    for (size_t q = 0; q < n; ++q) {
        uint64_t w[2] = {0, 0};
        for (size_t t = 0; t < k; ++t) {  // step t = symbol k-1-t, two bits each from bit 0 of word 0 up
            const uint8_t s = kmers[q * k + k - 1 - t];
            if (s != 1 && s != 2 && s != 3 && s != 5) return MSBWT_ERR_INVALID_SYMBOL;
            w[t >> 5] |= uint64_t(s - 1 - (s >> 2)) << (2 * (t & 31));
        }
        for (size_t i = 0; i < words; ++i) out_words[q * words + i] = w[i];
    }
    return MSBWT_OK;
}

int msbwt_rle_set_batch_order(msbwt_rle *h, int mode) {
    if (!h || mode < -1 || mode > 1) return MSBWT_ERR_INVALID_ARG;
    return set_locked(h, h->wanted_order, mode);
}

int msbwt_rle_get_batch_order(const msbwt_rle *h) { return h ? h->wanted_order : 0; }

int msbwt_rle_batch_order_for(const msbwt_rle *ch, size_t k, size_t n) {
    if (!ch || !ch->loaded) return MSBWT_ERR_INVALID_ARG;
    Call c(ch);
    return order_pays(c.h, view_of(c.h), k, n) ? 1 : 0;
}

int msbwt_rle_constrain_ranges_device(const msbwt_rle *ch, const void *d_syms, const void *d_l, const void *d_h,
                                      size_t n, void *d_out_l, void *d_out_h, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open(n && (!d_syms || !d_l || !d_h || !d_out_l || !d_out_h), "null device pointer")) return rc;
    msbwt_rle *h = c.h;
    HIP_TRY(h, launch_constrain_ranges(view_of(h), static_cast<const uint8_t *>(d_syms),
                                       static_cast<const uint64_t *>(d_l), static_cast<const uint64_t *>(d_h), n,
                                       static_cast<uint64_t *>(d_out_l), static_cast<uint64_t *>(d_out_h),
                                       h->d_flags + kDeviceFlags, static_cast<hipStream_t>(hip_stream)));
    return MSBWT_OK;
}

int msbwt_rle_count_read_kmers_device(const msbwt_rle *ch, const void *d_reads, size_t read_len, size_t n_reads,
                                      size_t k, int ascii, void *d_out_fwd, void *d_out_rc, void *hip_stream) {
    Call c(ch);
    const bool bad = k < 1 || k > 64 || k > read_len || read_len > 0xFFFFFFFFull || (!d_out_fwd && !d_out_rc) || (n_reads && !d_reads);
    if (int rc = c.open(bad, "count_read_kmers needs 1 <= k <= min(64, read_len) and an output")) return rc;
    return launch_read_kmers_locked(c.h, d_reads, read_len, n_reads, k, ascii, d_out_fwd, d_out_rc,
                                    static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

int msbwt_rle_count_read_kmers(const msbwt_rle *ch, const uint8_t *reads, size_t read_len, size_t n_reads, size_t k,
                               int ascii, uint64_t *out_fwd, uint64_t *out_rc) {
    Call c(ch);  // (the lock is held throughout: the staging buffer is per handle)
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (k < 1 || k > 64 || k > read_len || read_len > 0xFFFFFFFFull || (!out_fwd && !out_rc) || (n_reads && !reads))
        return fail(h, MSBWT_ERR_INVALID_ARG, "count_read_kmers needs 1 <= k <= min(64, read_len) and an output");
    if (int rc = c.loaded()) return rc;
    if (int rc = c.bind()) return rc;
    const size_t windows = read_len - k + 1;
    // pipelined: chunks of reads holding ~2 Mi windows travel host -> pinned -> HBM -> pinned -> host
    const size_t chunk = std::max<size_t>(1, (size_t(1) << 21) / windows);
    std::vector<HostArray> outs;
    if (out_fwd) outs.push_back(host_out(out_fwd, windows * sizeof(uint64_t)));
    if (out_rc) outs.push_back(host_out(out_rc, windows * sizeof(uint64_t)));
    return run_host_batch(h, n_reads, chunk, {host_in(reads, read_len)}, outs, "count_read_kmers", [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
        void *d_f = out_fwd ? d_out[0] : nullptr, *d_c = out_rc ? d_out[out_fwd ? 1 : 0] : nullptr;
        return launch_read_kmers_locked(h, d_in[0], read_len, m, k, ascii, d_f, d_c, stream, kHostFlags);
    });
}

int msbwt_rle_count_ragged_read_kmers(const msbwt_rle *ch, const uint8_t *reads, const uint64_t *read_offsets,
                                      size_t n_reads, size_t k, int ascii, uint64_t *out_fwd, uint64_t *out_rc,
                                      uint64_t *out_windows) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (k < 1 || k > 64 || (n_reads && (!read_offsets || !reads)))
        return fail(h, MSBWT_ERR_INVALID_ARG, "count_ragged_read_kmers needs 1 <= k <= 64 and offsets");
    // window prefix: read r owns [win[r], win[r+1])
    std::vector<uint64_t> win(n_reads + 1, 0);
    for (size_t r = 0; r < n_reads; ++r) {
        if (read_offsets[r + 1] < read_offsets[r]) return fail(h, MSBWT_ERR_INVALID_ARG, "read offsets must not decrease");
        const uint64_t len = read_offsets[r + 1] - read_offsets[r];
        win[r + 1] = win[r] + (len >= k ? len - k + 1 : 0);
    }
    const uint64_t total_windows = win[n_reads];
    if (out_windows) *out_windows = total_windows;
    if (!out_fwd && !out_rc) return MSBWT_OK;
    if (int rc = c.loaded()) return rc;
    if (total_windows == 0) return MSBWT_OK;
    if (int rc = c.bind()) return rc;
    // batches of whole reads holding at most ~4 Mi windows (at least one read)
    uint32_t all_flags = 0;
    for (size_t r0 = 0; r0 < n_reads;) {
        size_t r1 = r0 + 1;
        while (r1 < n_reads && win[r1 + 1] - win[r0] <= (uint64_t(1) << 22)) ++r1;
        const uint64_t nwin = win[r1] - win[r0], nbytes = read_offsets[r1] - read_offsets[r0];
        const size_t m = r1 - r0;
        if (nwin) {
            const size_t off_bytes = (m + 1) * sizeof(uint64_t);
            const size_t read_bytes = (size_t(nbytes) + 15) / 16 * 16;
            int rc = ensure_stage(h, read_bytes + 2 * off_bytes + 2 * nwin * sizeof(uint64_t) + 64);
            if (rc) return rc;
            uint8_t *d_r = static_cast<uint8_t *>(h->d_stage);
            uint64_t *d_roff = reinterpret_cast<uint64_t *>(d_r + read_bytes);
            uint64_t *d_woff = d_roff + (m + 1), *d_f = d_woff + (m + 1), *d_c = d_f + nwin;
            std::vector<uint64_t> roff(m + 1), woff(m + 1);  // rebased to the batch
            for (size_t i = 0; i <= m; ++i) {
                roff[i] = read_offsets[r0 + i] - read_offsets[r0];
                woff[i] = win[r0 + i] - win[r0];
            }
            HIP_TRY(h, hipMemcpyAsync(d_r, reads + read_offsets[r0], nbytes, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(d_roff, roff.data(), off_bytes, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(d_woff, woff.data(), off_bytes, hipMemcpyHostToDevice, h->stream));
            rc = timed_with_tickets(h, h->stream, [&](const IndexView &v) {
                return launch_count_ragged_read_kmers(v, d_r, d_roff, d_woff, m, nwin, uint32_t(k), ascii != 0, out_fwd ? d_f : nullptr,
                                                      out_rc ? d_c : nullptr, h->d_flags, h->stream);
            });
            if (rc) return rc;
            if (out_fwd) HIP_TRY(h, hipMemcpyAsync(out_fwd + win[r0], d_f, nwin * 8, hipMemcpyDeviceToHost, h->stream));
            if (out_rc) HIP_TRY(h, hipMemcpyAsync(out_rc + win[r0], d_c, nwin * 8, hipMemcpyDeviceToHost, h->stream));
            uint32_t flags = 0;
            rc = read_flags(h, h->stream, kHostFlags, &flags);  // synchronises: roff/woff may go out of scope
            if (rc) return rc;
            all_flags |= flags;
        }
        r0 = r1;
    }
    return flags_to_code(h, all_flags);
}

int msbwt_rle_device_status(const msbwt_rle *ch, void *hip_stream) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (!h->d_flags) return MSBWT_OK;
    if (int rc = c.bind()) return rc;
    return status_of(h, static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

int msbwt_rle_count_kmers(const msbwt_rle *ch, const uint8_t *kmers, size_t k, size_t n, uint64_t *out_counts) {
    Call c(ch);
    if (int rc = c.open(n && (!out_counts || (!kmers && k)), "null pointer")) return rc;
    if (n == 0) return MSBWT_OK;
    msbwt_rle *h = c.h;
    if (n <= kMailQueries && n * k <= kMailKmerBytes) {
        // the trait's single-query shape (msbwt_core.rs:124: one k-mer per call) and other tiny batches: through the
        // mailbox.  Every error ends its query with u64::MAX -- no real count is that large -- so the status word is
        // only read back when one shows up.
        if (int rc = ensure_mail(h)) return rc;
        const uint64_t *counts = reinterpret_cast<const uint64_t *>(h->mail + kMailCounts);
        if (!tier_launch_ok(h)) return hip_fail(h, hipErrorInvalidValue, "two-tier sparse table beside a direct table it cannot fall back to");
        IndexView v = view_of(h);  // no ticket counters: at most one tile
        // The lanes kernel announces completion in the mailbox itself; a single query even travels inside the kernel arguments.
        const bool poll = k <= 0xFFFFFFFFull && lanes_serves(v, uint32_t(k));
        const bool inlined = poll && n == 1;
        if (k && !inlined) std::memcpy(h->mail + kMailKmers, kmers, n * k);
        auto launch = [&] {
            return launch_count_kmers(v, h->d_mail + kMailKmers, uint32_t(k), n, reinterpret_cast<uint64_t *>(h->d_mail + kMailCounts), h->d_flags + kHostFlags,
                                      h->stream, inlined ? kmers : nullptr);
        };
        return mailbox_call(h, v, poll, [&] { return timed_launch(h, h->stream, launch); }, [&] {
            bool flagged = false;
            for (size_t i = 0; i < n; ++i) {
                out_counts[i] = counts[i];
                flagged |= counts[i] == ~0ull;
            }
            return flagged;
        });
    }
    // pipelined: chunks of 2 Mi queries travel host -> pinned -> HBM -> pinned -> host, copies and
    // kernels overlapping on three streams (host_pipeline.hpp)
    return run_host_batch(h, n, size_t(1) << 21, {host_in(kmers, k)}, {host_out(out_counts, sizeof(uint64_t))}, "count_kmers",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              return launch_count(h, static_cast<const uint8_t *>(d_in[0]), k, m, static_cast<uint64_t *>(d_out[0]), stream, kHostFlags);
                          });
}

int msbwt_rle_constrain_ranges(const msbwt_rle *ch, const uint8_t *syms, const uint64_t *l, const uint64_t *hh,
                               size_t n, uint64_t *out_l, uint64_t *out_h) {
    Call c(ch);
    if (int rc = c.open(n && (!syms || !l || !hh || !out_l || !out_h), "null pointer")) return rc;
    if (n == 0) return MSBWT_OK;
    msbwt_rle *h = c.h;
    if (n <= kMailQueries) {  // BWT::constrain_range, one range per call (msbwt_core.rs:99): through the mailbox, as above
        if (int rc = ensure_mail(h)) return rc;
        std::memcpy(h->mail + kMailSyms, syms, n);
        std::memcpy(h->mail + kMailL, l, n * sizeof(uint64_t));
        std::memcpy(h->mail + kMailH, hh, n * sizeof(uint64_t));
        IndexView v = view_of(h);
        const bool poll = n <= 8;  // one wave of 8-lane groups: the kernel announces completion in the mailbox
        auto launch = [&] {
            HIP_TRY(h, launch_constrain_ranges(v, h->d_mail + kMailSyms, reinterpret_cast<const uint64_t *>(h->d_mail + kMailL),
                                               reinterpret_cast<const uint64_t *>(h->d_mail + kMailH), n, reinterpret_cast<uint64_t *>(h->d_mail + kMailOutL),
                                               reinterpret_cast<uint64_t *>(h->d_mail + kMailOutH), h->d_flags + kHostFlags, h->stream));
            return int(MSBWT_OK);
        };
        return mailbox_call(h, v, poll, launch, [&] {
            const uint64_t *ol = reinterpret_cast<const uint64_t *>(h->mail + kMailOutL), *oh = reinterpret_cast<const uint64_t *>(h->mail + kMailOutH);
            bool flagged = false;
            for (size_t i = 0; i < n; ++i) {
                out_l[i] = ol[i];
                out_h[i] = oh[i];
                flagged |= ol[i] == ~0ull;  // an invalid symbol or range ends as {u64::MAX, u64::MAX}
            }
            return flagged;
        });
    }
    return run_host_batch(h, n, size_t(1) << 21, {host_in(syms, 1), host_in(l, sizeof(uint64_t)), host_in(hh, sizeof(uint64_t))},
                          {host_out(out_l, sizeof(uint64_t)), host_out(out_h, sizeof(uint64_t))}, "constrain_ranges",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              const hipError_t e = launch_constrain_ranges(view_of(h), static_cast<const uint8_t *>(d_in[0]), static_cast<const uint64_t *>(d_in[1]),
                                                                           static_cast<const uint64_t *>(d_in[2]), m, static_cast<uint64_t *>(d_out[0]),
                                                                           static_cast<uint64_t *>(d_out[1]), h->d_flags + kHostFlags, stream);
                              return e == hipSuccess ? int(MSBWT_OK) : hip_fail(h, e, "constrain_ranges pipeline");
                          });
}

int msbwt_rle_constrain_range(const msbwt_rle *h, uint8_t sym, uint64_t l, uint64_t hh, uint64_t *out_l,
                              uint64_t *out_h) {
    if (!out_l || !out_h) return MSBWT_ERR_INVALID_ARG;
    return msbwt_rle_constrain_ranges(h, &sym, &l, &hh, 1, out_l, out_h);
}

int msbwt_rle_count_kmer(const msbwt_rle *h, const uint8_t *kmer, size_t k, uint64_t *out_count) {
    if (!out_count) return MSBWT_ERR_INVALID_ARG;
    return msbwt_rle_count_kmers(h, kmer, k, 1, out_count);
}

int msbwt_rle_kmer_ranges_device(const msbwt_rle *ch, const void *d_kmers, size_t k, size_t n, void *d_out_l, void *d_out_h, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open(n && (!d_out_l || !d_out_h || (!d_kmers && k)), "null device pointer")) return rc;
    return launch_ranges(c.h, static_cast<const uint8_t *>(d_kmers), k, n, static_cast<uint64_t *>(d_out_l), static_cast<uint64_t *>(d_out_h), 1u,
                         static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

int msbwt_rle_count_kmer_extensions_device(const msbwt_rle *ch, const void *d_kmers, size_t k, size_t n, void *d_out_counts, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open(n && (!d_out_counts || (!d_kmers && k)), "null device pointer")) return rc;
    return launch_extensions(c.h, static_cast<const uint8_t *>(d_kmers), k, n, static_cast<uint64_t *>(d_out_counts), static_cast<hipStream_t>(hip_stream),
                             kDeviceFlags);
}

// host forms: pipelined like msbwt_rle_count_kmers (chunks of 2 Mi queries, host_pipeline.hpp), no mailbox
int msbwt_rle_kmer_ranges(const msbwt_rle *ch, const uint8_t *kmers, size_t k, size_t n, uint64_t *out_l, uint64_t *out_h) {
    Call c(ch);
    if (int rc = c.open(n && (!out_l || !out_h || (!kmers && k)), "null pointer")) return rc;
    if (n == 0) return MSBWT_OK;
    return run_host_batch(c.h, n, size_t(1) << 21, {host_in(kmers, k)}, {host_out(out_l, sizeof(uint64_t)), host_out(out_h, sizeof(uint64_t))}, "kmer_ranges",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              return launch_ranges(c.h, static_cast<const uint8_t *>(d_in[0]), k, m, static_cast<uint64_t *>(d_out[0]),
                                                   static_cast<uint64_t *>(d_out[1]), 1u, stream, kHostFlags);
                          });
}

int msbwt_rle_count_kmer_extensions(const msbwt_rle *ch, const uint8_t *kmers, size_t k, size_t n, uint64_t *out_counts) {
    Call c(ch);
    if (int rc = c.open(n && (!out_counts || (!kmers && k)), "null pointer")) return rc;
    if (n == 0) return MSBWT_OK;
    return run_host_batch(c.h, n, size_t(1) << 21, {host_in(kmers, k)}, {host_out(out_counts, 6 * sizeof(uint64_t))}, "count_kmer_extensions",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              return launch_extensions(c.h, static_cast<const uint8_t *>(d_in[0]), k, m, static_cast<uint64_t *>(d_out[0]), stream, kHostFlags);
                          });
}

// ---- counts by source (source_index.hip): the rows of every merged input inside a k-mer's range ----
int msbwt_rle_count_kmers_by_source_device(const msbwt_rle *ch, const void *d_kmers, size_t k, size_t n, void *d_out_counts, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open()) return rc;
    if (int rc = need_sources(c.h)) return rc;
    if (n && (!d_out_counts || (!d_kmers && k))) return fail(c.h, MSBWT_ERR_INVALID_ARG, "null device pointer");
    if (n == 0) return MSBWT_OK;
    return launch_by_source(c.h, static_cast<const uint8_t *>(d_kmers), k, n, static_cast<uint64_t *>(d_out_counts), static_cast<hipStream_t>(hip_stream),
                            kDeviceFlags);
}

int msbwt_rle_count_kmers_by_source(const msbwt_rle *ch, const uint8_t *kmers, size_t k, size_t n, uint64_t *out_counts) {
    Call c(ch);
    if (int rc = c.open()) return rc;
    if (int rc = need_sources(c.h)) return rc;
    if (n && (!out_counts || (!kmers && k))) return fail(c.h, MSBWT_ERR_INVALID_ARG, "null pointer");
    if (n == 0) return MSBWT_OK;
    return run_host_batch(c.h, n, by_source_chunk(c.h), {host_in(kmers, k)}, {host_out(out_counts, c.h->sources.n_sources * sizeof(uint64_t))}, "count_kmers_by_source",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              return launch_by_source(c.h, static_cast<const uint8_t *>(d_in[0]), k, m, static_cast<uint64_t *>(d_out[0]), stream, kHostFlags);
                          });
}

int msbwt_rle_range_sources_device(const msbwt_rle *ch, const void *d_l, const void *d_h, size_t n, void *d_out_counts, void *hip_stream) {
    Call c(ch);
    if (int rc = c.open()) return rc;
    if (int rc = need_sources(c.h)) return rc;
    if (n && (!d_l || !d_h || !d_out_counts)) return fail(c.h, MSBWT_ERR_INVALID_ARG, "null device pointer");
    return launch_sources_of_ranges(c.h, static_cast<const uint64_t *>(d_l), static_cast<const uint64_t *>(d_h), n, static_cast<uint64_t *>(d_out_counts),
                                    static_cast<hipStream_t>(hip_stream), kDeviceFlags);
}

int msbwt_rle_range_sources(const msbwt_rle *ch, const uint64_t *l, const uint64_t *hh, size_t n, uint64_t *out_counts) {
    Call c(ch);
    if (int rc = c.open()) return rc;
    if (int rc = need_sources(c.h)) return rc;
    if (n && (!l || !hh || !out_counts)) return fail(c.h, MSBWT_ERR_INVALID_ARG, "null pointer");
    if (n == 0) return MSBWT_OK;
    return run_host_batch(c.h, n, by_source_chunk(c.h), {host_in(l, sizeof(uint64_t)), host_in(hh, sizeof(uint64_t))},
                          {host_out(out_counts, c.h->sources.n_sources * sizeof(uint64_t))}, "range_sources",
                          [&](size_t m, void *const *d_in, void *const *d_out, hipStream_t stream) {
                              return launch_sources_of_ranges(c.h, static_cast<const uint64_t *>(d_in[0]), static_cast<const uint64_t *>(d_in[1]), m,
                                                              static_cast<uint64_t *>(d_out[0]), stream, kHostFlags);
                          });
}

// ---- batch order keys (order.hip): sort a batch by them and it walks the index in ascending order -----------------------
int msbwt_kmer_order_keys(const uint8_t *kmers, size_t k, size_t n, uint64_t *out_keys) {
    if (k < 1 || k > 0xFFFFFFFFull || (n && (!kmers || !out_keys))) return MSBWT_ERR_INVALID_ARG;
    order_keys_host(kmers, uint32_t(k), n, out_keys);
    return MSBWT_OK;
}

int msbwt_rle_kmer_order_keys_device(const msbwt_rle *ch, const void *d_kmers, size_t k, size_t n, void *d_out_keys, void *hip_stream) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (k < 1 || k > 0xFFFFFFFFull || (n && (!d_kmers || !d_out_keys))) return fail(h, MSBWT_ERR_INVALID_ARG, "order keys need 1 <= k and buffers");
    if (int rc = c.bind()) return rc;
    HIP_TRY(h, launch_order_keys(static_cast<const uint8_t *>(d_kmers), uint32_t(k), n, static_cast<uint64_t *>(d_out_keys), static_cast<hipStream_t>(hip_stream)));
    return MSBWT_OK;
}

}  // extern "C"
