"""What the unitigs by source ARE (msbwt_rle_enumerate_[canonical_]unitig_graph_by_source): a few lines over strings.

One Counter of the k-windows per source; the unitigs of the union from the string oracles of test_gpu_unitigs.py and
test_gpu_canonical_unitigs.py, imported, not copied; row u = the sum, over the windows of seqs[u], of the per-source counters -- in
the canonical case with the counter at the window's reverse complement added, a window that is its own reverse complement counted
once.  Nothing here needs a GPU or the library."""
import numpy as np

from test_gpu_canonical_unitigs import canonical_unitigs_of_texts, rc
from test_gpu_kmer_graph import windows
from test_gpu_unitigs import unitigs_of_texts

U64 = np.uint64


def source_sums(sets, k, seqs, canonical):
    """the U x S matrix of the unitigs `seqs` of the union of the read sets `sets` (lists of str, one a source)"""
    counters = [windows(reads, k) for reads in sets]
    out = np.zeros((len(seqs), len(sets)), dtype=U64)
    for u, seq in enumerate(seqs):
        for i in range(len(seq) - k + 1):
            q = seq[i:i + k]
            for s, counter in enumerate(counters):
                out[u, s] += U64(counter[q] + (counter[rc(q)] if canonical and rc(q) != q else 0))
    return out


def unitigs_by_source(sets, k, min_count=1, min_edge=0, canonical=False):
    """(the string oracle's unitigs of the union, their matrix)"""
    union = [r for reads in sets for r in reads]
    unitigs = (canonical_unitigs_of_texts if canonical else unitigs_of_texts)(union, k, min_count, min_edge)
    return unitigs, source_sums(sets, k, unitigs["seqs"], canonical)


def source_sums_of_codes(sets, k, symbols, offsets, canonical):
    """source_sums for large sets, in numpy: `sets` are lists of arrays of symbol codes, the unitigs the columns `symbols` and
    `offsets` of an oracle (tests/graph_oracle.py); the per-source counters are test_scaled_copies.census_of_codes"""
    import graph_oracle as G
    from test_scaled_copies import census_of_codes
    two = np.searchsorted(G.SYMBOL, symbols).astype(U64)
    offsets = np.asarray(offsets, dtype=np.int64)
    nodes = np.diff(offsets) - (k - 1)
    out = np.zeros((len(nodes), len(sets)), dtype=U64)
    if len(nodes) == 0:
        return out
    words = np.zeros(len(two) - k + 1, dtype=U64)
    for j in range(k):
        words = (words << U64(2)) | two[j:len(two) - k + 1 + j]
    at = np.arange(len(words))
    unitig = np.searchsorted(offsets, at, side="right") - 1
    words = words[at + k <= offsets[unitig + 1]]  # the windows that lie inside one unitig, in unitig order
    assert len(words) == nodes.sum() and (nodes >= 1).all()
    starts = np.concatenate([[0], np.cumsum(nodes)[:-1]])
    mirrors = G.rc_words(words, k)
    for s, reads in enumerate(sets):
        sorted_words, counts = census_of_codes(reads, k) if len(reads) else (np.zeros(0, dtype=U64), np.zeros(0, dtype=U64))
        per_node = G.counts_of(words, sorted_words, counts)
        if canonical:
            per_node = per_node + np.where(mirrors != words, G.counts_of(mirrors, sorted_words, counts), U64(0))
        out[:, s] = np.add.reduceat(per_node, starts)
    return out


def deal(reads, S):
    """read i to source i mod S"""
    return [list(reads[s::S]) for s in range(S)]
