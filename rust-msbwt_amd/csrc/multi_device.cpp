// Several devices: replicas of one index, batches sharded over them, and the count gathers over RCCL (gather.hip).
// Calls the single-device entry points, launch_count and handle.hpp; a replica's parts are copies, never rebuilt here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "gather.hpp"
#include "handle.hpp"
#include "pair_index.hpp"
#include "plane_index.hpp"

namespace {

// scratch of the all-gathers (hipFree waits for the device: no gather still reads the old buffer)
int ensure_gather(msbwt_rle *h, size_t need) {
    if (need <= h->gather_bytes) return MSBWT_OK;
    if (h->d_gather) (void)hipFree(h->d_gather);
    h->d_gather = nullptr;
    h->gather_bytes = 0;
    HIP_TRY(h, hipMalloc(&h->d_gather, need));
    h->gather_bytes = need;
    return MSBWT_OK;
}

// contiguous shards starting at multiples of 16 items (16-byte aligned rows for any k; sharded.py has the same rule)
void shard_of(size_t n, size_t world, size_t rank, size_t *lo, size_t *hi) {
    const size_t units = (n + 15) / 16, base = units / world, extra = units % world;
    const size_t lo_u = rank * base + std::min(rank, extra), hi_u = lo_u + base + (rank < extra ? 1 : 0);
    *lo = std::min(n, lo_u * 16);
    *hi = std::min(n, hi_u * 16);
}

// a non-empty list of handles, none of them null
bool all_handles(const msbwt_rle *const *replicas, size_t n) {
    return replicas && n && std::all_of(replicas, replicas + n, [](const msbwt_rle *r) { return r != nullptr; });
}

// runs work(r) for every replica on its own host thread; returns the first non-zero code
template <class Work>
int on_every_replica(size_t n_replicas, Work &&work) {
    std::vector<int> rc(n_replicas, MSBWT_OK);
    std::vector<std::thread> threads;
    for (size_t r = 1; r < n_replicas; ++r) threads.emplace_back([&, r] { rc[r] = work(r); });
    rc[0] = work(0);
    for (auto &t : threads) t.join();
    for (int c : rc)
        if (c) return c;
    return MSBWT_OK;
}

}  // namespace

extern "C" {

// ---- several devices of one node: replicas of one index, batches sharded over them --------------
msbwt_rle *msbwt_rle_replicate(const msbwt_rle *csrc, int device) {
    Call c(csrc);
    msbwt_rle *src = c.h;
    if (!src || c.loaded()) return nullptr;
    msbwt_rle *h = msbwt_rle_new_on_device(src->bin_power, device);
    if (!h) return nullptr;
    static_cast<Settings &>(*h) = *src;
    h->block_format = src->block_format;
    auto give_up = [&](int /* code: its text is on src */) -> msbwt_rle * {
        msbwt_rle_free(h);
        return nullptr;
    };
    DeviceScope scope(h->device);
    if (!scope.ok()) return give_up(fail(src, MSBWT_ERR_HIP, scope.why()));
    if (ensure_runtime(h) != MSBWT_OK) return give_up(hip_fail(src, hipErrorUnknown, "replicate: runtime setup"));
    if (h->device != src->device) {  // direct GPU -> GPU copies (xGMI) when the pair allows it; staged by the runtime otherwise
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, h->device, src->device) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(src->device, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
    }
    // the parts by value, then every device buffer re-pointed at its copy on this device (none is this handle's before that)
    h->pair = src->pair;
    h->table = src->table;
    h->sparse = src->sparse;
    h->sparse2 = src->sparse2;
    h->sources = src->sources;
    const SourceSizes ssz = source_sizes(src->totals.total, src->sources.n_sources);
    const PairIndexSizes psz = pair_index_sizes(src->nblocks, src->pair.stride);
    struct Piece { const void *from; void **to; size_t bytes; };
    const Piece pieces[] = {
        {src->d_blocks, &h->d_blocks, size_t(src->nblocks) * kBlockBytes},
        {src->d_overflow, &h->d_overflow, size_t(src->overflow_bytes)},
        {src->table.entries, &h->table.entries, src->table.bytes},
        {src->table.side, &h->table.side, size_t(src->table.side_bytes)},
        {src->table.filter, reinterpret_cast<void **>(&h->table.filter), (size_t(1) << (2 * src->table.filter_depth)) / 8},
        {src->pair.blocks, &h->pair.blocks, psz.pair_block_bytes},
        {src->pair.super, &h->pair.super, psz.super_bytes},
        {src->sparse.lines, &h->sparse.lines, size_t(src->sparse.bytes)},
        {src->sparse.side, &h->sparse.side, size_t(src->sparse.side_bytes)},
        {src->sparse2.lines, &h->sparse2.lines, size_t(src->sparse2.bytes)},
        {src->sparse2.side, &h->sparse2.side, size_t(src->sparse2.side_bytes)},
        {src->sources.rows, &h->sources.rows, size_t(ssz.row_bytes)},
        {src->sources.checkpoints, &h->sources.checkpoints, size_t(ssz.checkpoint_bytes)},
    };
    for (const Piece &p : pieces) *p.to = nullptr;
    for (const Piece &p : pieces) {
        if (!p.bytes || !p.from) continue;
        hipError_t e = hipMalloc(p.to, p.bytes);
        if (e == hipSuccess) e = hipMemcpyPeerAsync(*p.to, h->device, p.from, src->device, p.bytes, h->stream);
        if (e != hipSuccess) return give_up(hip_fail(src, e, "replicate: copy index to the other device"));
    }
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return give_up(hip_fail(src, e, "replicate: copy index to the other device"));
    h->totals = src->totals;
    h->nblocks = src->nblocks;
    h->overflow_bytes = src->overflow_bytes;
    h->sparse_report = src->sparse_report;
    h->typical_width = src->typical_width;
    h->loaded = true;
    return h;
}

int msbwt_rle_count_kmers_multi(const msbwt_rle *const *replicas, size_t n_replicas, const uint8_t *kmers, size_t k, size_t n,
                                uint64_t *out_counts) {
    if (!all_handles(replicas, n_replicas) || (n && (!out_counts || (!kmers && k)))) return MSBWT_ERR_INVALID_ARG;
    // one host thread and one pinned pipeline per replica; every shard's counts land directly in the
    // caller's buffer -- the "gather" is the D2H copies themselves
    return on_every_replica(n_replicas, [&](size_t r) {
        size_t lo, hi;
        shard_of(n, n_replicas, r, &lo, &hi);
        return hi > lo ? msbwt_rle_count_kmers(replicas[r], kmers + lo * k, k, hi - lo, out_counts + lo) : MSBWT_OK;
    });
}

int msbwt_rle_count_read_kmers_multi(const msbwt_rle *const *replicas, size_t n_replicas, const uint8_t *reads, size_t read_len,
                                     size_t n_reads, size_t k, int ascii, uint64_t *out_fwd, uint64_t *out_rc) {
    if (!all_handles(replicas, n_replicas) || k < 1 || k > read_len) return MSBWT_ERR_INVALID_ARG;
    const size_t windows = read_len - k + 1;
    return on_every_replica(n_replicas, [&](size_t r) {
        size_t lo, hi;
        shard_of(n_reads, n_replicas, r, &lo, &hi);
        if (hi <= lo) return int(MSBWT_OK);
        return msbwt_rle_count_read_kmers(replicas[r], reads + lo * read_len, read_len, hi - lo, k, ascii,
                                          out_fwd ? out_fwd + lo * windows : nullptr, out_rc ? out_rc + lo * windows : nullptr);
    });
}

int msbwt_rle_count_kmers_multi_device(const msbwt_rle *const *replicas, size_t n_replicas, const void *d_kmers, size_t k, size_t n,
                                       void *d_out_counts) {
    if (!all_handles(replicas, n_replicas) || (n && (!d_out_counts || (!d_kmers && k)))) return MSBWT_ERR_INVALID_ARG;
    const int home = replicas[0]->device;
    const uint8_t *src = static_cast<const uint8_t *>(d_kmers);
    uint64_t *dst = static_cast<uint64_t *>(d_out_counts);
    // enqueue every shard on its replica's stream: shard in by peer copy, kernel, counts back by peer copy.  An
    // error ends the enqueueing but NOT the call: the replicas already at work are drained below before the
    // first error is returned, so that nothing still writes into d_out_counts when the caller gets it back.
    auto enqueue = [&](size_t r) -> int {
        msbwt_rle *h = const_cast<msbwt_rle *>(replicas[r]);
        size_t lo, hi;
        shard_of(n, n_replicas, r, &lo, &hi);
        if (hi <= lo) return MSBWT_OK;
        Call c(h);
        if (int rc = c.loaded()) return rc;
        if (int rc = c.bind()) return rc;
        const size_t m = hi - lo;
        // MSBWT_FORCE_PEER_COPIES=1: take the staging + peer-copy path even on the home device (tests on one GPU)
        static const bool force_peer = [] { const char *e = std::getenv("MSBWT_FORCE_PEER_COPIES"); return e && std::atoi(e) != 0; }();
        if (h->device == home && !(force_peer && r > 0)) return launch_count(h, src + lo * k, k, m, dst + lo, h->stream, kHostFlags);
        const size_t kmer_bytes = (m * k + 255) / 256 * 256;
        int rc = ensure_stage(h, kmer_bytes + m * sizeof(uint64_t));
        if (rc) return rc;
        uint8_t *d_k = static_cast<uint8_t *>(h->d_stage);
        uint64_t *d_c = reinterpret_cast<uint64_t *>(d_k + kmer_bytes);
        if (k) HIP_TRY(h, hipMemcpyPeerAsync(d_k, h->device, src + lo * k, home, m * k, h->stream));
        rc = launch_count(h, d_k, k, m, d_c, h->stream, kHostFlags);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpyPeerAsync(dst + lo, home, d_c, h->device, m * sizeof(uint64_t), h->stream));
        return MSBWT_OK;
    };
    int first = MSBWT_OK;
    for (size_t r = 0; r < n_replicas && !first; ++r) first = enqueue(r);
    // the counts are complete when every replica's stream has drained
    for (size_t r = 0; r < n_replicas; ++r) {
        Call c(replicas[r]);
        if (!c.h->stream) continue;
        int rc = c.bind();
        if (!rc) rc = status_of(c.h, c.h->stream, kHostFlags);
        if (rc && !first) first = rc;
    }
    return first;
}

// ---- one process per GPU: the final count gather over RCCL ------------------------------------------------
int msbwt_comm_get_unique_id(void *out_id) {
    std::string why;
    if (!out_id) return MSBWT_ERR_INVALID_ARG;
    return comm_unique_id(out_id, &why) ? MSBWT_OK : MSBWT_ERR_RCCL;
}

int msbwt_comm_init_rank(void **out_comm, int nranks, const void *id, int rank) {
    std::string why;
    if (!out_comm || !id || nranks < 1 || rank < 0 || rank >= nranks) return MSBWT_ERR_INVALID_ARG;
    if (!comm_init_rank(out_comm, nranks, id, rank, &why)) {
        std::fprintf(stderr, "[msbwt] msbwt_comm_init_rank: %s\n", why.c_str());
        return MSBWT_ERR_RCCL;
    }
    return MSBWT_OK;
}

int msbwt_comm_destroy(void *comm) {
    std::string why;
    if (!comm) return MSBWT_ERR_INVALID_ARG;
    return comm_destroy(comm, &why) ? MSBWT_OK : MSBWT_ERR_RCCL;
}

int msbwt_rle_allgather_counts(const msbwt_rle *ch, void *comm, const void *d_mine, size_t n_mine, void *d_all, int wire_bits,
                               void *hip_stream) {
    Call c(ch);
    msbwt_rle *h = c.h;
    if (!h) return MSBWT_ERR_INVALID_ARG;
    if (!comm || (wire_bits != 64 && wire_bits != 32 && wire_bits != 16) || (n_mine && (!d_mine || !d_all)))
        return fail(h, MSBWT_ERR_INVALID_ARG, "allgather_counts needs a communicator, buffers and a wire width of 64, 32 or 16 bits");
    int rc = c.bind();
    if (!rc) rc = ensure_runtime(h);
    if (rc) return rc;
    std::string why;
    const int nranks = comm_ranks(comm, &why);
    if (nranks < 1) return fail(h, MSBWT_ERR_RCCL, why);
    const size_t need = allgather_scratch_bytes(n_mine, nranks, wire_bits);
    if ((rc = ensure_gather(h, need))) return rc;
    const hipError_t e = allgather_counts(comm, nranks, static_cast<const uint64_t *>(d_mine), n_mine, static_cast<uint64_t *>(d_all), wire_bits,
                                          h->d_gather, h->d_flags + kDeviceFlags, static_cast<hipStream_t>(hip_stream), &why);
    if (e == hipSuccess) return MSBWT_OK;
    return why.empty() ? hip_fail(h, e, "all-gather of the counts") : fail(h, MSBWT_ERR_RCCL, why);
}

// One batch counted and gathered as a PIPELINE (a caller with a single batch otherwise sees kernel + gather + widening one after the other):
// the rank's shard is cut into pieces; piece i is searched on the caller's stream while the counts of piece i - 1 travel -- narrowed,
// ncclAllGather, placed -- on a second stream of the handle.
int msbwt_rle_count_kmers_allgather_device(const msbwt_rle *ch, void *comm, const void *d_kmers, size_t k, size_t n_mine, void *d_mine_counts, void *d_all,
                                           int wire_bits, int out_bits, int pieces, void *hip_stream) {
    Call c(ch);
    int rc = c.open(!comm || (wire_bits != 64 && wire_bits != 32 && wire_bits != 16) || (out_bits != 64 && out_bits != wire_bits) || pieces < 1 || pieces > 64 ||
                        k < 1 || (n_mine && (!d_kmers || !d_mine_counts || !d_all)),
                    "count_kmers_allgather needs a communicator, buffers, a wire width of 64 / 32 / 16 bits, counts left at that width or widened to 64, 1..64 pieces");
    if (!rc) rc = ensure_runtime(c.h);
    if (rc) return rc;
    if (n_mine == 0) return MSBWT_OK;
    msbwt_rle *h = c.h;
    std::string why;
    const int nranks = comm_ranks(comm, &why);
    if (nranks < 1) return fail(h, MSBWT_ERR_RCCL, why);
    if (!h->gather_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->gather_stream, hipStreamNonBlocking));
    while (h->piece_events.size() < size_t(pieces) + 1) {
        hipEvent_t e = nullptr;
        HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->piece_events.push_back(e);
    }
    const size_t need = allgather_pieces_scratch_bytes(n_mine, nranks, wire_bits);
    if ((rc = ensure_gather(h, need))) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    // pieces of whole 16-query units (rows of any k then start 16-byte aligned: the fast kernels), the last one takes what is left
    const size_t per = allgather_piece_queries(n_mine, pieces);  // (gather.hpp: at most `pieces` pieces, whatever n_mine)
    // the gather stream starts behind everything the caller has queued so far (its buffers may still be in use there)
    HIP_TRY(h, hipEventRecord(h->piece_events[size_t(pieces)], stream));
    HIP_TRY(h, hipStreamWaitEvent(h->gather_stream, h->piece_events[size_t(pieces)], 0));
    size_t piece = 0;
    for (size_t off = 0; off < n_mine; off += per, ++piece) {
        const size_t len = std::min(per, n_mine - off);
        if (piece >= size_t(pieces)) {  // (cannot happen: allgather_piece_queries cuts at most `pieces` pieces)
            rc = fail(h, MSBWT_ERR_INTERNAL, "count_kmers_allgather: more pieces than events");
            break;
        }
        rc = launch_count(h, static_cast<const uint8_t *>(d_kmers) + off * k, k, len, static_cast<uint64_t *>(d_mine_counts) + off, stream, kDeviceFlags);
        if (rc) break;
        hipError_t e = hipEventRecord(h->piece_events[piece], stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->gather_stream, h->piece_events[piece], 0);
        if (e != hipSuccess) {
            rc = hip_fail(h, e, "piece event");
            break;
        }
        e = allgather_piece(comm, nranks, static_cast<const uint64_t *>(d_mine_counts), n_mine, off, len, d_all, wire_bits, out_bits, h->d_gather,
                            h->d_flags + kDeviceFlags, h->gather_stream, &why);
        if (e != hipSuccess) {
            rc = why.empty() ? hip_fail(h, e, "all-gather of a piece of the counts") : fail(h, MSBWT_ERR_RCCL, why);
            break;
        }
    }
    // The caller's stream continues once the last piece has arrived -- also after an error in the middle: pieces already queued on the
    // gather stream still write d_gather and d_all, so the caller's stream must not run ahead of them (after an RCCL error the
    // communicator is unusable and other ranks may be left inside ncclAllGather: the caller tears the job down).
    const hipError_t j1 = hipEventRecord(h->piece_events[size_t(pieces)], h->gather_stream);
    const hipError_t j2 = j1 == hipSuccess ? hipStreamWaitEvent(stream, h->piece_events[size_t(pieces)], 0) : j1;
    if (j2 != hipSuccess) {
        (void)hipStreamSynchronize(h->gather_stream);
        if (!rc) rc = hip_fail(h, j2, "join of the gather stream");
    }
    return rc;
}

size_t msbwt_allgather_piece_queries(size_t n_mine, int pieces) { return allgather_piece_queries(n_mine, pieces); }

}  // extern "C"
