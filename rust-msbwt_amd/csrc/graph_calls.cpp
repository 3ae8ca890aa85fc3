// The k-mer graph calls of a loaded index (kmer_graph.hpp): the sorted dump with an edge byte per k-mer, in its host and its device
// form, and the table of (in, out) degrees.  The frame of a call and the graph's two walks are walk_call.hpp's; where the tail of the
// call's block lies is graph_layouts.hpp's.
#include "walk_call.hpp"

#include "graph_layouts.hpp"
#include "kmer_graph.hpp"

namespace {

Shape graph_shape(bool fill) { return Shape{fill, false, fill ? graph_tail_layout(0).bytes : 0, kRecordBytes}; }  // (fixed: the tail of no records)

// The dump (both forms) and the degree table (table != nullptr: no record outputs, *out_n = the nodes, *out_edge_count = the edges):
// the sorted dump's counting walk, then the staged walk with the edge pass behind it.
int kmer_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, bool host, void *out_kmers, void *out_counts, void *out_l, void *out_edges,
               uint64_t capacity, uint64_t *out_n, uint64_t *table, uint64_t *out_edge_count, hipStream_t stream) {
    const bool degrees = table != nullptr;
    Frame f(bwt, degrees ? "kmer_graph_degrees" : "enumerate_kmer_graph", k, host, stream);
    const GraphCut cut(min_count, min_edge);
    if (int rc = f.open(false, [&] { return cut.check(f, degrees ? table : out_n); })) return rc;
    msbwt_rle *h = f.h;
    if (out_edge_count) *out_edge_count = 0;
    if (degrees) std::fill(table, table + kGraphTableWords, 0ull);
    const bool fill = degrees || capacity != 0;  // (the degree table has no capacity to fall short)
    Column cols[] = {{out_kmers}, {out_counts}, {out_l}};
    GraphTailLayout at{};
    char *tail = nullptr;
    return two_pass(
        f, degrees ? ~0ull : capacity, out_n, "k-mers", false, [&](uint64_t *n) { return count_nodes(f, graph_shape(fill), cut, n); },
        [&](uint64_t n) -> int {
            // one allocation: the records staged for a host dump, and graph_tail_layout behind them
            at = graph_tail_layout(n);
            if (int rc = stage_records(f, cols, n, &capacity, "for the edge bytes and the records", at.bytes, &tail)) return rc;
            HIP_TRY(h, hipMemsetAsync(tail + at.zero_from, 0, at.bytes - at.zero_from, f.stream));
            return graph_edge_walk(f, cut, n, in<uint32_t>(tail, at.edge_words), cols[0].as<uint64_t>(), cols[1].as<uint64_t>(), cols[2].as<uint64_t>(), nullptr);
        },
        [&](uint64_t n) -> int {
            const uint32_t *edge_words = in<uint32_t>(tail, at.edge_words);
            if (degrees) {
                uint64_t *d_table = in<uint64_t>(tail, at.table);
                HIP_TRY(h, launch_graph_degrees(edge_words, n, d_table, f.stream));
                HIP_TRY(h, hipMemcpyAsync(table, d_table, kGraphTableWords * 8, hipMemcpyDeviceToHost, f.stream));
                if (int rc = status_of(h, f.stream, f.which)) return rc;  // synchronises
                uint64_t edges = 0;
                for (uint32_t i = 0; i < kGraphTableWords; ++i) edges += uint64_t(i / kGraphDegrees) * table[i];  // (the in-degrees; the out-degrees sum to the same)
                if (out_edge_count) *out_edge_count = edges;
                return MSBWT_OK;
            }
            if (out_edges) HIP_TRY(h, hipMemcpyAsync(out_edges, edge_words, n, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, f.stream));
            if (!host) HIP_TRY(h, hipStreamSynchronize(f.stream));  // (the last chunk's edge pass, and the scratch is freed on return)
            return copy_out(f, cols);
        });
}

}  // namespace

extern "C" {

int msbwt_rle_enumerate_kmer_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_kmers2bit, uint64_t *out_counts, uint64_t *out_l,
                                   uint8_t *out_edges, uint64_t capacity, uint64_t *out_n) {
    return kmer_graph(bwt, k, min_count, min_edge, true, out_kmers2bit, out_counts, out_l, out_edges, capacity, out_n, nullptr, nullptr, nullptr);
}

int msbwt_rle_enumerate_kmer_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_kmers2bit, void *d_out_counts, void *d_out_l,
                                          void *d_out_edges, uint64_t capacity, uint64_t *out_n, void *hip_stream) {
    return kmer_graph(bwt, k, min_count, min_edge, false, d_out_kmers2bit, d_out_counts, d_out_l, d_out_edges, capacity, out_n, nullptr, nullptr,
                      static_cast<hipStream_t>(hip_stream));
}

int msbwt_rle_kmer_graph_degrees(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_table, uint64_t *out_nodes, uint64_t *out_edges) {
    uint64_t unwanted[kGraphTableWords];
    return kmer_graph(bwt, k, min_count, min_edge, true, nullptr, nullptr, nullptr, nullptr, 0, out_nodes, out_table ? out_table : unwanted, out_edges, nullptr);
}

// the host dump of `records` nodes with words, counts and l
int msbwt_kmer_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes) {
    return plan(graph_shape(true), total_rows, free_hbm_bytes, records, graph_tail_layout(records).bytes - graph_tail_layout(0).bytes, device_bytes);
}

}  // extern "C"
