// The functions of walk_call.hpp that are no templates: the sum over a Shape, the record a call leaves on the handle, the scratch of a
// walk, and the walks several families run -- the staged one, the canonical one, and the two of the k-mer graph.
#include "walk_call.hpp"

#include "canonical.hpp"
#include "kmer_graph.hpp"

namespace msbwt_capi __attribute__((visibility("hidden"))) {  // (said here too: shape_bytes has no caller in another unit to hide it at the link)

static_assert(MSBWT_SPECTRUM_MIN_FRONTIER == kSpectrumMinFrontier && MSBWT_SPECTRUM_INFO_WORDS == 4 + kSpectrumMaxK + 1 + 3, "the header's constants");

uint64_t shape_bytes(const Shape &p, uint64_t total_rows, uint64_t frontier, uint64_t records) {
    return spectrum_work_bytes(frontier) + (p.rank ? spectrum_rank_bytes(total_rows) : 0) + (p.canonical ? frontier * kCanonicalStageBytes : 0) + p.fixed +
           records * p.record_bytes;
}

int plan(const Shape &p, uint64_t total_rows, uint64_t free_bytes, uint64_t records, uint64_t more, uint64_t *device_bytes) {
    if (total_rows >= kMaxSymbols || records >= kMaxSymbols) return MSBWT_ERR_TOO_LARGE;
    if (device_bytes) *device_bytes = shape_bytes(p, total_rows, spectrum_frontier_nodes(total_rows, free_bytes, 0), records) + more;
    return MSBWT_OK;
}

void Frame::record() {
    h->spectrum_scratch = arena.taken;
    uint64_t *w = h->spectrum_info;
    std::fill(w, w + MSBWT_SPECTRUM_INFO_WORDS, 0ull);
    w[0] = info.k;
    w[1] = info.seed_depth;
    w[2] = info.chunks;
    w[3] = info.retries;
    std::copy(info.nodes, info.nodes + kSpectrumMaxK + 1, w + 4);
    const uint64_t us = clock.us();
    w[37] = (us + 500) / 1000;
    w[38] = us;
    w[39] = info.descents;
}

SpectrumSeeds seeds_of(const Frame &f) {
    const DirectTable &t = f.h->table;
    if (t.entries && !t.packed && t.depth > 0 && size_t(t.depth) < f.k) return SpectrumSeeds{t.entries, t.depth};
    return SpectrumSeeds{};
}

int take_scratch(Frame &f, const Shape &p) {
    msbwt_rle *h = f.h;
    size_t free_bytes = 0, all_bytes = 0;
    HIP_TRY(h, hipMemGetInfo(&free_bytes, &all_bytes));
    const uint64_t total = h->totals.total;
    f.frontier = spectrum_frontier_nodes(total, free_bytes, h->spectrum_frontier);
    const uint64_t bytes = shape_bytes(p, total, f.frontier, 0);
    const std::string need = f.needs(bytes, false, "while it runs");
    if (free_bytes < bytes) return fail(h, MSBWT_ERR_HIP, need);
    if (int rc = f.take(&f.work, spectrum_work_bytes(f.frontier), need)) return rc;
    if (p.rank)
        if (int rc = f.take(&f.rank, spectrum_rank_bytes(total), need)) return rc;
    if (p.canonical) {
        if (int rc = f.take(&f.rc_words, f.frontier * 8, need)) return rc;
        if (int rc = f.take(&f.rc_counts, f.frontier * 8, need)) return rc;
        if (int rc = f.take(&f.totals, kCanonicalTotalWords * 8, need)) return rc;
    }
    return MSBWT_OK;
}

int staged_walk(Frame &f, uint64_t prune, unsigned long long *d_totals, uint32_t words, uint64_t *totals, const SpectrumChunkHook &per_chunk) {
    msbwt_rle *h = f.h;
    f.hook_rc = MSBWT_OK;
    if (d_totals) HIP_TRY(h, hipMemsetAsync(d_totals, 0, words * 8, f.stream));
    const hipError_t walked = spectrum_stage(view_of(h), seeds_of(f), uint32_t(f.k), prune, f.work, f.frontier, per_chunk, &f.info, f.stream);
    if (f.hook_rc) return f.hook_rc;
    HIP_TRY(h, walked);
    if (!d_totals) return MSBWT_OK;
    HIP_TRY(h, hipMemcpyAsync(totals, d_totals, words * 8, hipMemcpyDeviceToHost, f.stream));
    HIP_TRY(h, hipStreamSynchronize(f.stream));
    return MSBWT_OK;
}

int canonical_walk(Frame &f, uint64_t prune, CanonicalSink sink, uint64_t *totals) {
    sink.totals = f.totals;
    return staged_walk(f, prune, f.totals, kCanonicalTotalWords, totals, [&](const void *d_kmers, uint64_t m) {
        const hipError_t e = launch_canonical_rc(d_kmers, m, uint32_t(f.k), f.rc_words, f.stream);
        if (e != hipSuccess) return e;
        if ((f.hook_rc = launch_count_2bit(f.h, f.rc_words, f.k, size_t(m), f.rc_counts, f.stream, f.which)) != MSBWT_OK) return hipErrorUnknown;
        return launch_canonical_combine(d_kmers, f.rc_words, f.rc_counts, m, sink, f.stream);
    });
}

int count_nodes(Frame &f, const Shape &p, const GraphCut &cut, uint64_t *n) {
    if (int rc = take_scratch(f, p)) return rc;
    HIP_TRY(f.h, spectrum_count(view_of(f.h), seeds_of(f), uint32_t(f.k), cut.m, 0, f.work, f.frontier, f.rank, n, &f.info, f.stream));
    return MSBWT_OK;
}

int graph_edge_walk(Frame &f, const GraphCut &cut, uint64_t n, uint32_t *edge_words, uint64_t *kmers, uint64_t *counts, uint64_t *l, uint64_t *pred) {
    const IndexView v = view_of(f.h);
    const SpectrumRank r = spectrum_rank_view(f.rank, f.h->totals.total);
    const GraphSink sink{r.bitmap, r.prefix, edge_words, n, cut.me, kmers, counts, l, f.h->d_flags + f.which, pred};
    return staged_walk(f, cut.m, nullptr, 0, nullptr, [&](const void *d_nodes, uint64_t nodes) { return launch_graph_edges(v, d_nodes, nodes, sink, f.stream); });
}

uint64_t ceil_log2(uint64_t x) {
    uint64_t r = 0;
    while (r < 63 && (1ull << r) < x) ++r;
    return r;
}

}  // namespace msbwt_capi
