"""The k-mer graph, the unitigs and the canonical unitigs (csrc/kmer_graph.hip, csrc/unitigs.hip, csrc/canonical_unitigs.hip and their
drivers in csrc/graph_calls.cpp and csrc/unitig_calls.cpp) at the sizes where their loops go round, and on an index of more than 2^32 rows whose k-mer ranges lie
on both sides of row 2^32.  Every column is compared for equality with tests/graph_oracle.py, the numpy oracle that
tests/test_graph_oracle.py holds to the string oracles of the neighbouring files on the CPU; nothing expected comes from the library.

1. One read set of 9.0e6 symbols (`scale_reads`): a random genome tiled by 150-base reads, reads with one substitution each from both
   strands, a few N, circles written as C + C[:31], and a second random sequence of 600 000 bases tiled without errors, one chain longer
   than a grid-stride trip.  (It is tiled, not one read: the builder sorts every suffix by as many 21-symbol key words as the longest
   read has, so one 600 000-base read would cost 28 572 x 8 radix passes over 9.7e6 suffixes; the graph is the same.)  The test asserts
   from the oracle, before it calls the library, that the set passes every point at which a loop takes another trip:
   524 288 slots (the second grid-stride trip of every slot-strided kernel), 1 048 576 canonical slots (the second chunk of the edge
   counting), 2 097 152 slots (the second round of k_scan_tile_sums<2>) and 4 194 304 slots (the second trip of k_unitig_tile_sums and
   k_unitig_number), a unitig of more than 524 288 nodes (20 rounds of pointer jumping and more), more than 1000 unitigs of several
   nodes, more than 1000 branching nodes and a circular unitig.  The tile loops of k_sort_histogram and k_sort_scatter (csrc/radix_sort.hip) go
   round only beyond 2^20 tiles, 4.3e9 slots; they are reached at toy sizes under MSBWT_SORT_GRID, by
   test_gpu_canonical_unitigs.test_sort_grid_cap_gives_the_same_unitigs and test_gpu_reads_build.test_sort_grid_cap_*, not here.
2. S x 4096 for S = copy_set(1 100 000, 11, ...), the "past it" set of tests/test_gpu_scaled_copies.py with a few reads put in (below):
   4 505 600 000 rows.  The graph of S x c under thresholds times c is the graph of S with the counts, count sums and range starts
   times c (tests/test_graph_oracle.py and tests/test_scaled_copies.py prove it), so the oracle runs on 1.1e6 rows.  In
   copy_set(1 100 000, 11) as it is no k-mer's range has row 2^20 inside it, so nothing would straddle row 2^32.  The reads put in,
   1684 of the 1 100 000 rows, see to that in the manner of LIFT in tests/test_gpu_scaled_copies.py: ASTRIDE twice, a read whose
   last 31 symbols begin with a 12-mer that sorts some 200 rows past row 2^20, and LIFT reads TTT with four empty reads for each of the
   LIFT_ROOM - LIFT others, which choose row by row which suffix sits at row 2^20.  Both were found on the CPU by the oracle's ranges;
   the test asserts from the oracle that a 12-mer's and a 31-mer's range straddle row 2^32.
3. A homopolymer index of 4.8e9 rows whose node count, unitig count sum and canonical class count at k = 1 exceed 2^32.

Measured on a free MI355X (none of the cases skipped; the whole file 58 s, of which 17 s the numpy oracle and the CPU builder, 9.3 s
load_reads of the 4.5e9 symbols and 12 s the start of torch in the first test that wants it when the file runs alone):

* the first test of each part pays for what is made once: 10.7 s in test_graph_at_multi_trip_sizes[21] (the oracle of both k and the
  load), 8.8 s in test_graph_past_2_to_32[12] (the CPU builder on S and the load of S x 4096);
* the set: 60 012 reads, 9 007 572 symbols, load_reads 0.27 s (0.06 s for the flipped set, the buffers at hand);
* k = 21: 2 300 137 nodes, 2 335 605 edges, 130 254 unitigs, the longest 599 980 nodes, 6 circular, 43 rounds; under (2, 3) 969 863
  nodes, 232 193 unitigs, 38 rounds.  Canonical: 3 793 854 slots in 4 edge chunks, 1 896 927 classes, 126 420 unitigs, the longest
  580 919, 44 rounds; under (2, 3) 1 195 418 slots in 2 chunks, 195 898 unitigs, 40 rounds;
* k = 31: 2 623 464 nodes, 2 651 930 edges, 123 832 unitigs, the longest 599 970, 6 circular, 43 rounds; under (2, 3) 896 658 nodes,
  195 811 unitigs, 37 rounds.  Canonical: 4 444 144 slots in 5 edge chunks, 2 222 072 classes, 120 743 unitigs, the longest 599 970,
  44 rounds; under (2, 3) 1 083 494 slots in 2 chunks, 139 964 unitigs, 40 rounds;
* a call with its comparison 0.01 to 0.03 s under the automatic frontier (one chunk of the walk), 0.16 to 0.23 s under a frontier of
  65 536 (208 chunks; 16 under (2, 3)); the dump and the degree table of the graph 0.08 to 0.17 s; both _device forms 0.07 and 0.09 s;
  the properties without the oracle 0.8 s; the oracle 0.7 s (plain) and 2.3 to 2.9 s (canonical) a case;
* past 2^32, k = 12: 292 902 nodes, 17 590 ranges start past row 2^32, one straddles it, in-degree 1 below / past it 243 035 / 15 522;
  38 552 unitigs in 6 rounds, 289 544 classes in 43 568 canonical unitigs; under (8192, 0) 10 788 nodes in 3 634 unitigs.  k = 31:
  15 894 nodes, 934 past, one astride, 11 875 / 746; 3 273 unitigs in 4 rounds.  The graph tests 1.2 s (without the load) and 4.6 s,
  the unitig tests 0.4 s and 4.7 s, the canonical 12-mers 4.6 s, the count sum past 2^32 (4 845 000 000 rows) 5.5 s.

Sensitivity, with two libraries built apart for that and not kept, each changing values only and forming no address from them:
k_edge_words reading keys[j] for keys[first + j] fails every canonical test of the first part, the _device and the property test
(S = 21 844 207 for 4 425 327 at k = 21) and passes the graph and the plain unitigs; k_scan_tile_sums<2> with its carry dropped fails
every plain and canonical unitig test of the first part with wrong symbols in arrays of the right size -- the numbers it hands out
stay below U and S, so the numbering's guards do not see it -- and passes the graph.  Every test passes with the library as it is:
this file found no fault in the kernels or the driver.
"""
import importlib
import math
import time

import numpy as np
import pytest

import graph_oracle as G
from test_gpu_canonical_unitigs import INFO, check_properties
from test_gpu_kmer_graph import check_graph
from test_gpu_merge_many import homopolymer_rle
from test_gpu_scaled_copies import BUILDS, COPIES, EDGE, free_or_skip, rle_of
from test_gpu_sparse import oracle_ranges
from test_gpu_unitigs import check_unitigs
from test_scaled_copies import EMPTY, U64, bwt_symbols, copy_set, tiled

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
unpack_2bit = msbwt.rle_bwt.unpack_2bit

TRIP = 2048 * 256          # slots one launch of a slot-strided kernel covers without going round (kGridCap workgroups of 256)
EDGE_CHUNK = 1 << 20       # kCanonicalUnitigChunkSlots
SCAN_ROUND = 1024 * 2048   # slots k_scan_tile_sums<2> covers in one round of 1024 tiles
TILE_TRIP = 2048 * 2048    # slots k_unitig_tile_sums and k_unitig_number cover with one tile a workgroup
KS = (21, 31)
PAIRS = ((1, 0), (2, 3))
FRONTIERS = {"automatic frontier": 0, "frontier 65536": 1 << 16}
GENOME, ERROR_READS, CHAIN, READ, STEP, CIRCLE, CIRCLES, WITH_N = 400000, 50000, 600000, 150, 100, 600, 6, 40


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---- 1. the read set of the multi-trip sizes, its oracle and its two indexes, each made once ----

def scale_reads():
    """the read set as a list of arrays of symbol codes"""
    rng = np.random.default_rng(2024)
    genome, chain = G.SYMBOL[rng.integers(0, 4, size=GENOME)], G.SYMBOL[rng.integers(0, 4, size=CHAIN)]
    span = np.arange(READ)
    tiles = lambda text: text[np.append(np.arange(0, text.size - READ, STEP), text.size - READ)[:, None] + span[None, :]]
    # one substitution each, from random places of the genome; every third from the other strand; N in place of the first few
    errors = genome[rng.integers(0, GENOME - READ + 1, size=ERROR_READS)[:, None] + span[None, :]]
    at = rng.integers(0, READ, size=ERROR_READS)
    value = (np.searchsorted(G.SYMBOL, errors[np.arange(ERROR_READS), at]) + rng.integers(1, 4, size=ERROR_READS)) % 4
    errors[np.arange(ERROR_READS), at] = G.SYMBOL[value]
    errors[np.arange(WITH_N), at[:WITH_N]] = 4
    errors[::3] = G.FLIP[errors[::3, ::-1]]
    reads = list(tiles(genome)) + list(errors) + list(tiles(chain))
    for i in range(CIRCLES):  # circles; the first half of them three times, so that they outlast the thresholds (2, 3)
        c = G.SYMBOL[rng.integers(0, 4, size=CIRCLE)]
        reads += [np.concatenate([c, c[:max(KS)]])] * (3 if i < CIRCLES // 2 else 1)
    return reads


_scale = {}


def scale_set():
    if "reads" not in _scale:
        _scale["reads"] = scale_reads()
    return _scale["reads"]


def scale_want(kind, k, pair):
    """the oracle's graph ("graph"), unitigs ("plain") or canonical unitigs ("canonical") of the set, computed once"""
    if ("census", k) not in _scale:
        _scale["census", k] = G.census(scale_set(), k)
    if (kind, k, pair) not in _scale:
        t0 = time.perf_counter()
        if kind == "canonical" and ("classes", k) not in _scale:
            _scale["classes", k] = G.canonical_census(_scale["census", k], k)
        make = {"graph": G.graph_of_census, "plain": G.unitigs_of_census, "canonical": G.canonical_unitigs_of_census}[kind]
        _scale[kind, k, pair] = make(_scale["census", k], k, *pair, *([_scale["classes", k]] if kind == "canonical" else []))
        print("oracle: %s, k = %d, %s: %.1f s" % (kind, k, pair, time.perf_counter() - t0))
    return _scale[kind, k, pair]


def scale_sizes():
    """What makes this set the test it is, asserted from the oracle's own numbers before any call into the library."""
    if "sizes" not in _scale:
        plain = {k: scale_want("plain", k, (1, 0)) for k in KS}
        canonical = {k: scale_want("canonical", k, (1, 0)) for k in KS}
        assert plain[31]["info"]["nodes"] > SCAN_ROUND
        assert canonical[31]["slots"] > TILE_TRIP and canonical[31]["slots"] == 2 * canonical[31]["info"]["classes"] - canonical[31]["info"]["palindromes"]
        assert canonical[21]["slots"] > 3 * EDGE_CHUNK  # several chunks of the edge counting
        for k in KS:
            for want in (plain[k], canonical[k]):
                lengths = np.diff(want["offsets"].astype(np.int64)) - (k - 1)
                assert want["info"]["longest"] == lengths.max() > TRIP
                assert (lengths > 1).sum() >= 1000 and want["info"]["circular"] >= 1
            assert plain[k]["branching"] >= 1000
            assert scale_want("plain", k, (2, 3))["info"]["nodes"] > TRIP and scale_want("plain", k, (2, 3))["info"]["circular"] >= 1
        _scale["sizes"] = True
    return True


def scale_index(flipped):
    """a handle with the set loaded by load_reads, as it is or with every second read reverse-complemented"""
    if ("index", flipped) not in _scale:
        scale_sizes()
        reads = G.flip_every_second(scale_set()) if flipped else scale_set()
        offsets = np.zeros(len(reads) + 1, dtype=U64)
        np.cumsum([r.size for r in reads], out=offsets[1:])
        t0 = time.perf_counter()
        b = msbwt.RleBWT(device=0)
        b.load_reads((np.concatenate(reads), offsets))
        assert b.get_total_size() == int(offsets[-1]) + len(reads)
        print("load_reads of %d reads, %d symbols%s: %.2f s" % (len(reads), int(offsets[-1]), ", every second read flipped" if flipped else "", time.perf_counter() - t0))
        _scale["index", flipped] = b
    return _scale["index", flipped]


def rounds_hold(rounds, slots, longest):
    """the project's bound on the rounds of the ranking; a node 2^19 links from its head is reached by no fewer than 20 doublings"""
    assert rounds <= 3 * (math.ceil(math.log2(slots)) + 1) if slots > 1 else rounds == 0, (rounds, slots)
    if longest > TRIP:
        assert rounds >= 20, (rounds, longest)


def same_columns(got, want, where):
    for name, g in zip(G.NAMES, got):
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (where, name, g.shape, want[name].shape)
        bad = np.flatnonzero(g != want[name])
        assert bad.size == 0, (where, name, bad[:5], g[bad[:5]], want[name][bad[:5]])


def check_canonical_columns(b, k, want, min_count, min_edge, where):
    got = b.enumerate_canonical_unitigs(k, min_count=min_count, min_edge=min_edge or None)
    same_columns(got, want, where)
    info = b.canonical_unitig_info()
    assert {x: info[x] for x in INFO} == want["info"], (where, info, want["info"])
    rounds_hold(info["rounds"], want["slots"], want["info"]["longest"])
    return got, info


@pytest.mark.parametrize("k", KS)
def test_graph_at_multi_trip_sizes(k):
    scale_sizes()
    b = scale_index(False)
    for pair in PAIRS:
        t0 = time.perf_counter()
        words, counts, edges, n_edges = scale_want("graph", k, pair)
        assert len(words) > TRIP
        check_graph(b, k, (words, counts, None, edges, n_edges), *pair)  # the dump, then the degree table
        print("graph, k = %d, %s: %d nodes, %d edges, %.2f s" % (k, pair, len(words), n_edges, time.perf_counter() - t0))


@pytest.mark.parametrize("frontier", sorted(FRONTIERS))
@pytest.mark.parametrize("k", KS)
def test_unitigs_at_multi_trip_sizes(k, frontier):
    scale_sizes()
    b = scale_index(False)
    b.set_spectrum_frontier(FRONTIERS[frontier])
    try:
        for pair in PAIRS:
            t0 = time.perf_counter()
            want = scale_want("plain", k, pair)
            check_unitigs(b, k, want, *pair)
            info, chunks = b.unitig_info(), b.spectrum_info()["chunks"]
            rounds_hold(info["rounds"], info["nodes"], want["info"]["longest"])
            assert chunks >= (want["info"]["nodes"] >> 16 if FRONTIERS[frontier] else 1)
            print("unitigs, k = %d, %s, %s: %d nodes, %d unitigs, the longest %d, %d circular, %d rounds, %d chunks of the walk, %.2f s"
                  % (k, pair, frontier, info["nodes"], info["unitigs"], info["longest"], info["circular"], info["rounds"], chunks, time.perf_counter() - t0))
    finally:
        b.set_spectrum_frontier(0)


@pytest.mark.parametrize("strands", ["as loaded", "every second read flipped"])
@pytest.mark.parametrize("frontier", sorted(FRONTIERS))
@pytest.mark.parametrize("k", KS)
def test_canonical_unitigs_at_multi_trip_sizes(k, frontier, strands):
    scale_sizes()
    b = scale_index(strands != "as loaded")
    b.set_spectrum_frontier(FRONTIERS[frontier])
    try:
        for pair in PAIRS:
            t0 = time.perf_counter()
            want = scale_want("canonical", k, pair)  # the strand-merged graph does not know which strand a read came from
            _, info = check_canonical_columns(b, k, want, *pair, where=(k, pair, frontier, strands))
            print("canonical unitigs, k = %d, %s, %s, %s: %d slots in %d edge chunks, %d classes, %d unitigs, the longest %d, %d circular, %d rounds, %.2f s"
                  % (k, pair, frontier, strands, want["slots"], -(-want["slots"] // EDGE_CHUNK), info["classes"], info["unitigs"], info["longest"], info["circular"],
                     info["rounds"], time.perf_counter() - t0))
    finally:
        b.set_spectrum_frontier(0)


def device_columns(call, U, S):
    """the five columns of a _device entry point, from torch tensors of exactly U and S entries"""
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    bufs = [torch.zeros(S, dtype=torch.uint8, device=dev), torch.zeros(U + 1, dtype=torch.int64, device=dev), torch.zeros(U, dtype=torch.int64, device=dev),
            torch.zeros(U, dtype=torch.uint8, device=dev), torch.zeros(U, dtype=torch.uint8, device=dev)]
    assert call(*[x.data_ptr() for x in bufs], U, S, stream=stream) == (U, S)
    return [x.cpu().numpy().view(U64) if x.dtype == torch.int64 else x.cpu().numpy() for x in bufs]


def test_device_entry_points_at_multi_trip_sizes():
    import torch
    scale_sizes()
    b, k = scale_index(False), 31
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    for kind, device, host in (("plain", b.enumerate_unitigs_device, b.enumerate_unitigs), ("canonical", b.enumerate_canonical_unitigs_device, b.enumerate_canonical_unitigs)):
        t0 = time.perf_counter()
        want = scale_want(kind, k, (1, 0))
        U, S = device(k, None, None, None, None, None, 0, 0, stream=stream)  # the counting call sizes the tensors
        assert (U, S) == (want["info"]["unitigs"], want["info"]["symbols"])
        got = device_columns(lambda *a, **kw: device(k, *a, **kw), U, S)
        b.device_status(stream)
        same_columns(got, want, (kind, "device"))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, host(k)))
        print("%s unitigs into device buffers, k = %d: %d unitigs, %d symbols, %.2f s" % (kind, k, U, S, time.perf_counter() - t0))


def test_properties_that_need_no_oracle_at_multi_trip_sizes():
    scale_sizes()
    b, k = scale_index(False), 31
    t0 = time.perf_counter()
    got = b.enumerate_canonical_unitigs(k)
    assert len(got[2]) == scale_want("canonical", k, (1, 0))["info"]["unitigs"]
    check_properties(b, k, got)  # S = n + U (k - 1); no unitig beside its mirror; the count sums through count_ragged_read_kmers
    print("properties of %d canonical unitigs, k = %d: %.2f s" % (len(got[2]), k, time.perf_counter() - t0))


# ---- 2. a scattered index beyond 2^32 rows ----

BIG_KS = (12, 31)
BIG_PAIRS = {(1, 0): (1, 0), (2 * COPIES, 0): (2, 0), (2 * COPIES, 3 * COPIES): (2, 3), (2 * COPIES - 1, 0): (2, 0)}  # on S x c: on S
ASTRIDE, LIFT, LIFT_ROOM = "CCGACTTACCTTACGACTAGGCGTGGGCGAGTAAAACCATA", 208, 400
_big = {}


def big_set():
    """(S, the CPU builder's BWT symbols of it), made once"""
    if "set" not in _big:
        rows, _ = BUILDS["past it"]
        ttt = np.array([5, 5, 5], dtype=np.uint8)
        reads = copy_set(rows, 11, G.codes_of_texts([ASTRIDE, ASTRIDE]) + [ttt] * LIFT + [EMPTY] * (4 * (LIFT_ROOM - LIFT)))
        assert sum(r.size + 1 for r in reads) == rows == 1100000
        symbols = bwt_symbols(reads)
        symbols.setflags(write=False)
        _big["set"] = (reads, symbols)
    return _big["set"]


def big_want(orc, kind, k, pair=None):
    """the oracle on S, computed once; "ranges" = (words, l) of all k-mers of S by the CPU oracle's search"""
    reads, symbols = big_set()
    if ("census", k) not in _big:
        _big["census", k] = G.census(reads, k)
        ref = orc.OracleRleBWT()
        ref.load_vector(rle_of(symbols))
        words, counts = _big["census", k][:2]
        l, h = oracle_ranges(ref, unpack_2bit(words, k))
        assert np.array_equal(h - l, counts)  # (the oracle agrees with the census)
        _big["ranges", k] = (words, l)
    if (kind, k, pair) not in _big and kind != "ranges":
        make = {"graph": G.graph_of_census, "plain": G.unitigs_of_census, "canonical": G.canonical_unitigs_of_census}[kind]
        _big[kind, k, pair] = make(_big["census", k], k, *pair)
    return _big["ranges", k] if kind == "ranges" else _big[kind, k, pair]


def big_index():
    """S x 4096 in run blocks, loaded once"""
    if "index" not in _big:
        rows, c = BUILDS["past it"]
        total = rows * c
        assert c == COPIES and total == 4505600000 > EDGE
        free_or_skip("load_reads of %d symbols" % total, 8 * total)
        reads, _ = big_set()
        flat, offsets = tiled(reads, c)
        b = msbwt.RleBWT(device=0)
        b.set_block_format("runs")
        t0 = time.perf_counter()
        b.load_reads((flat, offsets))
        print("load_reads of %d symbols: %.2f s" % (total, time.perf_counter() - t0))
        del flat, offsets
        assert b.get_block_format() == "runs" and b.get_total_size() == total == 4505600000
        small = np.bincount(np.concatenate(reads), minlength=6)
        small[0] = len(reads)
        assert [b.get_symbol_count(s) for s in range(6)] == [c * int(x) for x in small]
        _big["index"] = b
    return _big["index"]


@pytest.mark.parametrize("k", BIG_KS)
def test_graph_past_2_to_32(orc, k):
    t0 = time.perf_counter()
    c = U64(COPIES)
    all_words, all_l = big_want(orc, "ranges", k)
    wants = {big: big_want(orc, "graph", k, small) for big, small in BIG_PAIRS.items()}
    words, counts, edges, _ = wants[1, 0]
    l = all_l * c
    past, straddling = l > EDGE, (l < EDGE) & (l + counts * c > EDGE)
    in_degree_1 = G.POP[edges & 15] == 1
    print("k = %d: %d nodes, %d ranges start past 2^32, %d straddle it, in-degree 1 below / past: %d / %d"
          % (k, len(words), int(past.sum()), int(straddling.sum()), int((in_degree_1 & ~past).sum()), int((in_degree_1 & past).sum())))
    assert past.sum() > (10 ** 4 if k == 12 else 500)
    assert straddling.sum() >= 1
    assert (in_degree_1 & ~past).any() and (in_degree_1 & past).any()
    b = big_index()
    for (m, me), small in BIG_PAIRS.items():
        words, counts, edges, n_edges = wants[m, me]
        keep = np.isin(all_words, words, assume_unique=True)
        assert keep.sum() == len(words) and (small == (1, 0)) == keep.all()
        check_graph(b, k, (words, counts * c, all_l[keep] * c, edges, n_edges), m, me)
    assert len(wants[1, 0][0]) > len(wants[2 * COPIES, 0][0]) > 100 and wants[2 * COPIES, 0][3] > wants[2 * COPIES, 3 * COPIES][3] > 0
    # a threshold past 2^32: no k-mer of this index occurs that often; cut to 32 bits it would be 1 and return them all
    assert int(wants[1, 0][1].max()) * COPIES < EDGE
    got = b.enumerate_kmer_graph(k, min_count=EDGE + 1, ranges=True)
    assert all(x.size == 0 for x in got)
    table, nodes, n_edges = b.kmer_graph_degrees(k, min_count=EDGE + 1)
    assert not table.any() and nodes == 0 and n_edges == 0
    for refused in (lambda: b.enumerate_kmer_graph(k, min_count=EDGE + 1, min_edge=EDGE), lambda: b.kmer_graph_degrees(k, min_count=EDGE + 1, min_edge=EDGE)):
        with pytest.raises(MsbwtError) as err:
            refused()
        assert err.value.code == _lib.ERR_INVALID_ARG and "min_edge" in str(err.value)
    print("graph past 2^32, k = %d: %.2f s" % (k, time.perf_counter() - t0))


@pytest.mark.parametrize("k", BIG_KS)
def test_unitigs_past_2_to_32(orc, k):
    t0 = time.perf_counter()
    wants = {big: (big_want(orc, "plain", k, small), big_want(orc, "canonical", k, small)) for big, small in BIG_PAIRS.items()}
    assert wants[1, 0][0]["info"]["unitigs"] > wants[2 * COPIES, 0][0]["info"]["unitigs"] > 10
    b = big_index()
    for (m, me), (plain, canonical) in wants.items():
        check_unitigs(b, k, G.scaled(plain, COPIES), m, me)
        plain_info = b.unitig_info()
        _, info = check_canonical_columns(b, k, G.scaled(canonical, COPIES), m, me, where=(k, m, me))
        print("past 2^32, k = %d, (%d, %d): %d nodes in %d unitigs, %d rounds; %d classes in %d canonical unitigs, %d rounds"
              % (k, m, me, plain_info["nodes"], plain_info["unitigs"], plain_info["rounds"], info["classes"], info["unitigs"], info["rounds"]))
    for call, report in ((b.enumerate_unitigs, b.unitig_info), (b.enumerate_canonical_unitigs, b.canonical_unitig_info)):
        got = call(k, min_count=EDGE + 1)
        assert [len(a) for a in got] == [0, 1, 0, 0, 0] and got[1].tolist() == [0] and not any(report().values())
        with pytest.raises(MsbwtError) as err:
            call(k, min_count=EDGE + 1, min_edge=EDGE)
        assert err.value.code == _lib.ERR_INVALID_ARG and "min_edge" in str(err.value)
    print("unitigs past 2^32, k = %d: %.2f s" % (k, time.perf_counter() - t0))


def test_canonical_kmers_past_2_to_32(orc):
    t0 = time.perf_counter()
    k, c = 12, U64(COPIES)
    big_want(orc, "ranges", k)
    cen = _big["census", k]
    both, cc = G.class_census(cen[0], cen[1], k)
    assert both.size > cen[0].size  # (k-mers seen on one strand only)
    mirror = G.rc_words(both, k)
    smaller = both <= mirror
    own, other = G.counts_of(both, cen[0], cen[1]), np.where(mirror == both, U64(0), G.counts_of(mirror, cen[0], cen[1]))
    assert np.array_equal(own + other, cc) and (other[smaller] > 0).sum() > 100
    b = big_index()
    for m, small in ((1, 1), (2 * COPIES, 2), (2 * COPIES - 1, 2)):
        keep = smaller & (cc >= U64(small))
        got = b.enumerate_canonical_kmers(k, min_count=m, sorted=True, strands=True)
        assert 100 < keep.sum() and (small == 1 or keep.sum() < smaller.sum())
        assert np.array_equal(got[0], both[keep]) and np.array_equal(got[1], own[keep] * c) and np.array_equal(got[2], other[keep] * c), (m, len(got[0]), int(keep.sum()))
    assert all(x.size == 0 for x in b.enumerate_canonical_kmers(k, min_count=EDGE + 1))
    print("canonical 12-mers past 2^32: %d classes, %.2f s" % (int(smaller.sum()), time.perf_counter() - t0))


# ---- 3. a count sum past 2^32 ----

def homopolymer_unitigs(reads, length, min_count):
    """k = 1 over reads c^length: the node c occurs reads[c] * length times and c.c, its only edge, reads[c] * (length - 1) times; a
    node is a unitig of its own, circular where its self-loop counts.  Strand-merged, A and T are one class and C and G another, and
    A.T, C.G are no edges: the unitigs A and C.  -> (plain, canonical) as (symbols, offsets, count sums, ends, flags)"""
    count = {x: reads[x] * length for x in "ACGT"}
    loop = {x: reads[x] * (length - 1) for x in "ACGT"}
    for x, y in ("AT", "CG"):
        count[x + y], loop[x + y] = count[x] + count[y], loop[x] + loop[y]

    def columns(kept):
        linked = [int(loop[x] >= min_count) for x in kept]
        return (np.array([G.CODE_OF[x[0]] for x in kept], dtype=np.uint8), np.arange(len(kept) + 1, dtype=U64), np.array([count[x] for x in kept], dtype=U64),
                np.array([(0x11 << "ACGT".index(x[0])) * on for x, on in zip(kept, linked)], dtype=np.uint8), np.array(linked, dtype=np.uint8))

    return columns([x for x in "ACGT" if count[x] >= min_count]), columns([x for x in ("AT", "CG") if count[x] >= min_count])


def test_a_count_sum_past_2_to_32(tmp_path):
    t0 = time.perf_counter()
    length, k = 29, 1
    # the closed form, held to the oracle on a set small enough to write out
    few = {"A": 3, "C": 5, "G": 7, "T": 2}
    codes = [np.full(length, G.CODE_OF[x], dtype=np.uint8) for x in "ACGT" for _ in range(few[x])]
    for min_count in (1, 5 * (length - 1) + 1, 5 * length, 5 * length + 1, 12 * (length - 1) + 1, 12 * length + 1):
        plain, canonical = homopolymer_unitigs(few, length, min_count)
        for want, got in ((plain, G.unitigs_of_codes(codes, k, min_count)), (canonical, G.canonical_unitigs_of_codes(codes, k, min_count))):
            assert all(np.array_equal(x, got[name]) for x, name in zip(want, G.NAMES)), (min_count, want, got)
    reads = {"A": 3 * 10 ** 5, "C": 5 * 10 ** 5, "G": 7 * 10 ** 5, "T": 16 * 10 ** 7}
    total = sum(reads.values()) * (length + 1)
    assert reads["T"] * length == 4640000000 > reads["T"] * (length - 1) == 4480000000 > EDGE and total == 4845000000
    assert reads["A"] * length < EDGE and (reads["C"] + reads["G"]) * length < EDGE
    free_or_skip("index of %d rows" % total, 8 * total)
    b = msbwt.RleBWT(device=0)
    b.load_vector(homopolymer_rle(reads, length, str(tmp_path / "homopolymers.npy")))
    assert b.get_total_size() == total
    # every node and class; only what is past 2^32; T's loop gone, T left; T gone, the class of A and T left without its loop; nothing
    cases = ((1, 4, 4, 2, 2), (EDGE + 1, 1, 1, 1, 1), (reads["T"] * (length - 1) + 1, 1, 0, 1, 1), (reads["T"] * length + 1, 0, 0, 1, 0),
             ((reads["T"] + reads["A"]) * length + 1, 0, 0, 0, 0))
    for min_count, n_plain, loops_plain, n_canonical, loops_canonical in cases:
        plain, canonical = homopolymer_unitigs(reads, length, min_count)
        assert (len(plain[2]), int(plain[4].sum()), len(canonical[2]), int(canonical[4].sum())) == (n_plain, loops_plain, n_canonical, loops_canonical), min_count
        if min_count <= EDGE + 1:
            assert plain[2].max() > EDGE and canonical[2].max() > plain[2].max() and plain[4].all() and canonical[4].all()
        got = b.enumerate_unitigs(k, min_count=min_count)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, plain)), (min_count, got, plain)
        info = b.unitig_info()
        if n_plain:
            assert {x: info[x] for x in info if x != "rounds"} == {"nodes": n_plain, "edges": loops_plain, "links": loops_plain, "unitigs": n_plain, "symbols": n_plain,
                                                                   "circular": loops_plain, "longest": 1}, (min_count, info)
        else:
            assert not any(info.values())
        words, counts, edges = b.enumerate_kmer_graph(k, min_count=min_count)
        assert words.tolist() == ["ACGT".index(x) for x in "ACGT" if reads[x] * length >= min_count]
        assert np.array_equal(counts, plain[2]) and np.array_equal(edges, plain[3])  # the single self-loop of every node
        got = b.enumerate_canonical_unitigs(k, min_count=min_count)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, canonical)), (min_count, got, canonical)
        info = b.canonical_unitig_info()
        if n_canonical:
            assert {x: info[x] for x in INFO} == {"classes": n_canonical, "edge_classes": loops_canonical, "links": loops_canonical, "unitigs": n_canonical,
                                                  "symbols": n_canonical, "circular": loops_canonical, "longest": 1, "palindromes": 0, "cut_links": 0}, (min_count, info)
        else:
            assert not any(info.values())
    print("a count sum past 2^32: %.2f s" % (time.perf_counter() - t0))
