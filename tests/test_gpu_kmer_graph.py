"""The k-mer graph (csrc/kmer_graph.hip, csrc/graph_calls.cpp): the sorted dump with an edge byte per k-mer, and the degree table.

Expected values never come from the code under test: a census of the reads' ACGT-only windows at k and at k + 1 -- a Counter over
strings for the small sets (and for k = 32, where k + 1 does not fit a word), numpy for the 4000-read sets --, the CPU oracle's ranges
for every l and its count_kmer for spot checks of single bits, and closed forms for homopolymer reads.

Shapes: ragged sets of 1-50 reads of 0-70 symbols with N, duplicates and prefixes, and hand-made sets with a read of exactly k and of
k + 1 symbols, a k-mer preceded only by '$' or 'N' and a self-loop; the 20 000-base genome's read sets with 0.5 % errors (4.0e5
symbols) under several thresholds; a frontier cap at its minimum, where the successor bits land on records of other chunks; every
index form; one index beyond 2^32 rows.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib
from collections import Counter

import numpy as np
import pytest

from test_gpu_merge_many import EMPTY, homopolymer_rle
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_sparse import oracle_ranges
from test_gpu_spectrum import census_of_matrix, loaded, oracle_of, word_of

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
unpack_2bit = msbwt.rle_bwt.unpack_2bit
U64 = np.uint64
KS = (1, 2, 3, 4, 15, 16, 17, 30, 31, 32)
THRESHOLDS = ((1, 0), (2, 0), (2, 2), (1, 3), (3, 7), (10 ** 9, 0))  # (min_count, min_edge); the last gives n = 0


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def thresholds(min_count, min_edge):
    m = max(min_count, 1)
    return m, (min_edge if min_edge else m)


# ---- the census: what the graph of a read set IS, from its windows alone ----

def windows(reads, k):
    return Counter(r[i:i + k] for r in reads for i in range(len(r) - k + 1) if set(r[i:i + k]) <= set("ACGT"))


def graph_of_texts(reads, k, min_count=1, min_edge=0):
    """(words, counts, edge bytes, number of edges) of reads given as strings: Counters over the windows of k and of k + 1 symbols."""
    m, me = thresholds(min_count, min_edge)
    nodes = sorted((word_of(q), n, q) for q, n in windows(reads, k).items() if n >= m)
    solid = {e for e, n in windows(reads, k + 1).items() if n >= me}
    edges = [sum(1 << j for j in range(4) if "ACGT"[j] + q in solid) | sum(16 << j for j in range(4) if q + "ACGT"[j] in solid) for _, _, q in nodes]
    return (np.array([x[0] for x in nodes], dtype=U64), np.array([x[1] for x in nodes], dtype=U64), np.array(edges, dtype=np.uint8), len(solid))


def graph_of_census(words, counts, words1, counts1, k, min_count=1, min_edge=0):
    """the same from the numpy censuses at k (words, counts) and at k + 1 <= 32 (words1, counts1)"""
    m, me = thresholds(min_count, min_edge)
    keep = counts >= U64(m)
    words, counts = words[keep], counts[keep]
    solid = words1[counts1 >= U64(me)]
    edges = np.zeros(len(words), dtype=np.uint8)
    mask = U64((1 << (2 * k)) - 1)
    # e = j.q: a predecessor bit of q = e[1..k]; e = p.j: a successor bit of p = e[0..k)
    for node, sym, shift in ((solid & mask, solid >> U64(2 * k), 0), (solid >> U64(2), solid & U64(3), 4)):
        at = np.searchsorted(words, node)
        assert len(solid) == 0 or (at < len(words)).all() and np.array_equal(words[at], node)  # both ends of an edge are nodes
        np.bitwise_or.at(edges, at, (np.uint8(1) << (sym.astype(np.uint8) + np.uint8(shift))))
    return words, counts, edges, len(solid)


_census = {}


def read_set_graph(orc, name, k, min_count=1, min_edge=0):
    """(words, counts, l, edge bytes, number of edges) of read_set(name): the censuses and the oracle's ranges, computed once per (name, k)"""
    if (name, k) not in _census:
        (flat, offsets), rle = read_set(name)
        matrix = flat.reshape(-1, int(offsets[1]))
        words, counts = census_of_matrix(matrix, k)
        l, h = oracle_ranges(oracle_of(orc, rle), unpack_2bit(words, k))
        assert np.array_equal(h - l, counts)  # (the oracle agrees with the census)
        for a in (words, counts, l):
            a.setflags(write=False)
        _census[name, k] = (words, counts, l) + census_of_matrix(matrix, k + 1)
    words, counts, l, words1, counts1 = _census[name, k]
    w, c, e, n_edges = graph_of_census(words, counts, words1, counts1, k, min_count, min_edge)
    return w, c, l[counts >= U64(max(min_count, 1))], e, n_edges


def degree_table(edges):
    """np.bincount over the (in, out) degrees of the edge bytes"""
    pop = np.array([bin(x).count("1") for x in range(16)], dtype=np.int64)
    return np.bincount(5 * pop[edges & 15] + pop[edges >> 4], minlength=25).astype(U64).reshape(5, 5)


def check_graph(b, k, want, min_count=1, min_edge=0):
    """the dump and the degree call against want = (words, counts, l or None, edges, number of edges)"""
    words, counts, l, edges, n_edges = want
    got = b.enumerate_kmer_graph(k, min_count=min_count, min_edge=min_edge or None, ranges=True)
    gw, gc, ge, gl = got
    assert gw.dtype == gc.dtype == gl.dtype == U64 and ge.dtype == np.uint8
    assert np.array_equal(gw, words), (k, min_count, min_edge, len(gw), len(words))
    assert np.array_equal(gc, counts), (k, min_count, min_edge)
    if l is not None:
        assert np.array_equal(gl, l), (k, min_count, min_edge, np.flatnonzero(gl != l)[:5])
    bad = np.flatnonzero(ge != edges)
    assert bad.size == 0, (k, min_count, min_edge, bad[:5], ge[bad[:5]], edges[bad[:5]])
    table, nodes, n = b.kmer_graph_degrees(k, min_count=min_count, min_edge=min_edge or None)
    want_table = degree_table(edges)
    assert table.dtype == U64 and table.shape == (5, 5) and np.array_equal(table, want_table), (k, min_count, min_edge, table, want_table)
    assert nodes == len(words) == int(table.sum())
    assert n == n_edges == int((table.sum(axis=1) * np.arange(5, dtype=U64)).sum()) == int((table.sum(axis=0) * np.arange(5, dtype=U64)).sum())
    return got


def with_ranges(orc, rle, k, graph):
    """graph_of_texts' tuple with the oracle's l of every node put in"""
    words, counts, edges, n_edges = graph
    l = np.zeros(0, dtype=U64)
    if len(words):
        l, h = oracle_ranges(oracle_of(orc, rle), unpack_2bit(words, k))
        assert np.array_equal(h - l, counts)
    return words, counts, l, edges, n_edges


# ---- 1. exactness on small sets ----

@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets_at_every_k(orc, seed):
    reads = ragged_set(seed)
    rle = naive_rle(orc, reads)
    b = loaded(rle)
    seen = 0
    for k in KS:
        want = with_ranges(orc, rle, k, graph_of_texts(reads, k))
        check_graph(b, k, want)
        check_graph(b, k, with_ranges(orc, rle, k, graph_of_texts(reads, k, 2, 0)), 2, 0)
        seen += int((want[3] != 0).sum())
    assert seen > 50  # (the sets do have edges)


def test_hand_made_sets_and_single_bits_by_the_oracle(orc):
    k = 5
    reads = ["ACGTA",             # a read of exactly k symbols: a node with no edge
             "GGCATC",            # a read of k + 1: one edge, GGCAT -> GCATC
             "TTGACNCCGTTA",      # TTGAC is preceded only by '$', CCGTT only by 'N'; ...GAC N: no successor across the N
             "CCGTTAG",           # ... and here CCGTT follows '$'
             "AAAAAAAA",          # the self-loop AAAAA -> AAAAA
             "TGGCATCAAAAAG", "TGGCATG"]  # a branch: GGCAT -> GCATC and GCATG, GGCAT <- TGGCA
    rle = naive_rle(orc, reads)
    b, ref = loaded(rle), oracle_of(orc, rle)
    want = with_ranges(orc, rle, k, graph_of_texts(reads, k))
    words, counts, edges, l = check_graph(b, k, want)[0], want[1], want[3], want[2]
    byte = dict(zip(words.tolist(), edges.tolist()))
    bit = lambda sym, successor=False: (16 if successor else 1) << "ACGT".index(sym)
    assert byte[word_of("ACGTA")] == 0
    assert byte[word_of("GGCAT")] == bit("T") | bit("C", True) | bit("G", True) and byte[word_of("GCATC")] == bit("G") | bit("A", True)
    assert byte[word_of("TTGAC")] == 0 and byte[word_of("CCGTT")] == bit("A", True) and byte[word_of("TGGCA")] == bit("T", True)
    assert byte[word_of("AAAAA")] == bit("A") | bit("C") | bit("A", True) | bit("G", True)
    # every bit of every node is count_kmer of the (k+1)-mer against the threshold, by the oracle
    got = b.enumerate_kmer_graph(k, min_count=1, min_edge=2)[2]
    for q, e1, e2 in zip(words.tolist(), edges.tolist(), got.tolist()):
        text = "".join("ACGT"[(q >> (2 * (k - 1 - i))) & 3] for i in range(k))
        for j, sym in enumerate("ACGT"):
            before, after = ref.count_kmer(orc.convert_stoi(sym + text)), ref.count_kmer(orc.convert_stoi(text + sym))
            assert ((e1 >> j) & 1, (e1 >> (4 + j)) & 1) == (int(before >= 1), int(after >= 1)), (text, sym)
            assert ((e2 >> j) & 1, (e2 >> (4 + j)) & 1) == (int(before >= 2), int(after >= 2)), (text, sym)
    for kk in (4, 6, 7, 8, 12, 13):  # k at and around the lengths of the reads
        check_graph(b, kk, with_ranges(orc, rle, kk, graph_of_texts(reads, kk)))
    assert b.enumerate_kmer_graph(14)[0].size == 0


# ---- 2. thresholds ----

@pytest.mark.parametrize("k", [15, 31])
@pytest.mark.parametrize("name", ["plain_100", "repeat_150"])
def test_thresholds_on_read_sets_with_errors(orc, name, k):
    _, rle = read_set(name)
    b = loaded(rle)
    sizes = []
    for min_count, min_edge in THRESHOLDS:
        want = read_set_graph(orc, name, k, min_count, min_edge)
        check_graph(b, k, want, min_count, min_edge)
        sizes.append((len(want[0]), want[4]))
    print("%s, k = %d: (nodes, edges) per threshold %s" % (name, k, sizes))
    assert sizes[-1] == (0, 0) and sizes[0][0] > sizes[1][0] > sizes[4][0] > 100 and sizes[0][1] > sizes[3][1] > 100 and sizes[1][1] == sizes[2][1]
    table = degree_table(read_set_graph(orc, name, k)[3])
    assert table[1, 1] > 1000 and table[1, 2] + table[2, 1] > 10  # (the errors branch the graph)
    for form in (lambda: b.enumerate_kmer_graph(k, min_count=3, min_edge=2), lambda: b.kmer_graph_degrees(k, min_count=3, min_edge=2)):
        with pytest.raises(MsbwtError) as err:
            form()
        assert err.value.code == _lib.ERR_INVALID_ARG and "min_edge" in str(err.value)


# ---- 3. chunks: the successor bits land on records of other chunks ----

@pytest.mark.parametrize("k", [15, 31])
@pytest.mark.parametrize("name", ["plain_100", "repeat_150"])
def test_a_frontier_at_its_minimum_gives_the_same_bytes(orc, name, k):
    _, rle = read_set(name)
    b = loaded(rle)
    want = read_set_graph(orc, name, k)
    auto = check_graph(b, k, want)
    auto_info = b.spectrum_info()
    assert auto_info["retries"] == 0 and auto_info["descents"] == 0
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)
    first = b.enumerate_kmer_graph(k, ranges=True)
    info = b.spectrum_info()  # the writing walk
    second = b.enumerate_kmer_graph(k, ranges=True)
    print("%s, k = %d, frontier %d: %d chunks, %d retries, %d descents, %.1f ms" % (name, k, _lib.SPECTRUM_MIN_FRONTIER, info["chunks"], info["retries"],
                                                                                    info["descents"], info["ms"]))
    assert info["k"] == k and info["chunks"] >= 1000 and info["retries"] >= 1 and info["nodes"][k] == len(want[0])
    for x, y, z in zip(first, second, auto):
        assert np.array_equal(x, z) and np.array_equal(y, z)
    table, nodes, edges = b.kmer_graph_degrees(k)
    assert np.array_equal(table, degree_table(want[3])) and nodes == len(want[0]) and edges == want[4]
    b.set_spectrum_frontier(0)


# ---- 4. every index form gives the same answer ----

FORMS = {"defaults": dict(), "no pair index": dict(pair_index=0), "pair stride 96": dict(pair_index=1, pair_stride=96),
         "flat table seeds the walk": dict(pair_index=0, table_depth=5), "run blocks": dict(block_format="runs")}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_index_form_gives_the_same_answer(orc, form):
    name = "repeat_150"
    _, rle = read_set(name)
    knobs = FORMS[form]
    b = loaded(rle, **knobs)
    assert b.get_block_format() == knobs.get("block_format", "planes")
    if "pair_index" in knobs:
        assert b.get_pair_index() == bool(knobs["pair_index"])
    if "pair_stride" in knobs:
        assert b.get_pair_stride() == knobs["pair_stride"]
    for k in (15, 31):
        check_graph(b, k, read_set_graph(orc, name, k))
        check_graph(b, k, read_set_graph(orc, name, k, 2, 3), 2, 3)
        seed_depth = b.spectrum_info()["seed_depth"]
        print("%s, k = %d: seed depth %d" % (form, k, seed_depth))
        if form in ("no pair index", "flat table seeds the walk"):
            assert 0 < seed_depth < k
        if form == "flat table seeds the walk":
            assert seed_depth == b.get_table_depth() == 5


# ---- 5. degrees: closed forms ----

def test_degrees_of_homopolymers_and_of_an_empty_index(tmp_path):
    reads, length = {"A": 5, "C": 3, "G": 2, "T": 4}, 6
    b = loaded(homopolymer_rle(reads, length, str(tmp_path / "homopolymers.npy")))
    for k in range(1, length + 2):
        # c^k occurs n_c (length - k + 1) times, c^(k+1) n_c (length - k) times: every node its own only neighbour while k < length
        for min_count in (1, 2 * (length - k + 1) + 1, 5 * (length - k + 1) + 1):
            nodes = [c for c in "ACGT" if k <= length and reads[c] * (length - k + 1) >= min_count]
            linked = [c for c in nodes if k < length and reads[c] * (length - k) >= min_count]
            table, n, edges = b.kmer_graph_degrees(k, min_count=min_count)
            want = np.zeros((5, 5), dtype=U64)
            want[1, 1], want[0, 0] = len(linked), len(nodes) - len(linked)
            assert np.array_equal(table, want) and n == len(nodes) and edges == len(linked), (k, min_count, table)
            w, c, e = b.enumerate_kmer_graph(k, min_count=min_count)
            assert w.tolist() == [word_of(x * k) for x in nodes] and c.tolist() == [reads[x] * (length - k + 1) for x in nodes]
            assert e.tolist() == [0x11 << "ACGT".index(x) if x in linked else 0 for x in nodes]
    table, n, edges = b.kmer_graph_degrees(3)
    assert np.count_nonzero(table) == 1 and table[1, 1] == 4  # one non-zero cell
    empty = loaded(EMPTY)
    for k in (1, 21, 32):
        table, n, edges = empty.kmer_graph_degrees(k)
        assert not table.any() and n == 0 and edges == 0
        assert all(x.size == 0 for x in empty.enumerate_kmer_graph(k, ranges=True))


# ---- 6. capacity, NULL buffers, scratch ----

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_capacity_and_null_buffers(orc):
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    name, k, min_count = "plain_100", 17, 2
    _, rle = read_set(name)
    words, counts, l, edges, _ = read_set_graph(orc, name, k, min_count)
    want = {"w": words, "c": counts, "l": l, "e": edges}
    n = len(words)
    assert n > 100
    b = loaded(rle)
    lib, got_n = _lib.lib(), C.c_uint64(0)
    total, before, free = b.get_total_size(), b.device_bytes(), torch.cuda.mem_get_info(0)[0]
    plan = lambda records: msbwt.kmer_graph_plan(total, free, records)
    assert plan(0) == msbwt.kmer_graph_plan(total, 10 ** 9, 0) and total + 1024 < 2 ** 20  # the frontier is the index's, not the memory's

    def host(capacity, skip=()):
        bufs = {"w": np.full(n + 2, 7, dtype=U64), "c": np.full(n + 2, 7, dtype=U64), "l": np.full(n + 2, 7, dtype=U64), "e": np.full(n + 2, 7, dtype=np.uint8)}
        args = [_ptr(bufs[x]) if x not in skip else None for x in "wcle"]
        return lib.msbwt_rle_enumerate_kmer_graph(b._h, k, min_count, 0, *args, capacity, C.byref(got_n)), bufs

    # the two-call pattern; a capacity too small writes nothing and names n
    rc, bufs = host(0)
    assert rc == 0 and got_n.value == n and all((a == 7).all() for a in bufs.values())
    assert b.spectrum_scratch_bytes() == msbwt.spectrum_plan(total, free, 0, False)  # counting marks nothing
    for capacity in (1, n - 1):
        got_n.value = 0
        rc, bufs = host(capacity)
        assert rc == _lib.ERR_INVALID_ARG and got_n.value == n and str(n).encode() in lib.msbwt_rle_last_error(b._h)
        assert all((a == 7).all() for a in bufs.values())
    # every output NULL in turn, and all at once
    for skip in ((), ("w",), ("c",), ("l",), ("e",), ("w", "c", "l", "e")):
        rc, bufs = host(n + 1, skip)
        assert rc == 0 and got_n.value == n, skip
        for x in "wcle":
            assert (bufs[x][n:] == 7).all() and (np.array_equal(bufs[x][:n], want[x]) if x not in skip else (bufs[x] == 7).all()), (skip, x)
        assert b.spectrum_scratch_bytes() == plan(n) - 8 * n * len(set(skip) & set("wcl")), skip
    # the device form: the same, into buffers of the caller's; the edge bytes at an odd address
    assert b.enumerate_kmer_graph_device(k, None, None, None, None, 0, min_count=min_count, stream=stream) == n
    for skip in ((), ("w",), ("c",), ("l",), ("e",)):
        bufs = {x: torch.full((n + 3,), -7, dtype=torch.int64, device=dev) for x in "wcl"}
        bufs["e"] = torch.full((n + 9,), 7, dtype=torch.uint8, device=dev)
        ptrs = [bufs[x].data_ptr() if x not in skip else None for x in "wcl"] + [bufs["e"].data_ptr() + 1 if "e" not in skip else None]
        assert (bufs["e"].data_ptr() + 1) % 2 == 1
        with pytest.raises(MsbwtError) as err:
            b.enumerate_kmer_graph_device(k, *ptrs, n - 1, min_count=min_count, stream=stream)
        assert err.value.code == _lib.ERR_INVALID_ARG and err.value.n == n and str(n) in str(err.value)
        assert all(bool((bufs[x] == -7).all()) for x in "wcl") and bool((bufs["e"] == 7).all())
        assert b.enumerate_kmer_graph_device(k, *ptrs, n, min_count=min_count, stream=stream) == n
        b.device_status(stream)
        assert b.spectrum_scratch_bytes() == plan(n) - 24 * n  # no records staged
        for x in "wcl":
            got = bufs[x].cpu().numpy()
            assert (got[n:] == -7).all() and (np.array_equal(got[:n].astype(U64), want[x]) if x not in skip else (got == -7).all()), (skip, x)
        got = bufs["e"].cpu().numpy()
        assert got[0] == 7 and (got[n + 1:] == 7).all()  # nothing before the first byte, nothing after the n-th
        assert np.array_equal(got[1:n + 1], edges) if "e" not in skip else (got == 7).all()
    b.kmer_graph_degrees(k, min_count=min_count)
    assert b.spectrum_scratch_bytes() == plan(n) - 24 * n
    assert b.device_bytes() == before
    # the guards behind "nothing loaded"
    for bad_k in (0, 33, 1000):
        assert lib.msbwt_rle_enumerate_kmer_graph(b._h, bad_k, 1, 0, None, None, None, None, 0, C.byref(got_n)) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_enumerate_kmer_graph_device(b._h, bad_k, 1, 0, None, None, None, None, 0, C.byref(got_n), None) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_kmer_graph_degrees(b._h, bad_k, 1, 0, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmer_graph(b._h, k, 3, 2, None, None, None, None, 0, C.byref(got_n)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmer_graph(b._h, k, 0, 0, None, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmer_graph(b._h, k, 0, 1, None, None, None, None, 0, C.byref(got_n)) == 0  # min_count 0 is 1


# ---- 7. beyond 2^32 rows ----

def test_beyond_2_to_32_rows(tmp_path):
    """The homopolymer index of test_gpu_spectrum.test_beyond_2_to_32_rows, 4.5e9 rows, under a frontier cap: the nodes are c^k with
    c^(k+1) their only edge, a self-loop each; at k = 28 T's l lies beyond 2^32, so the checkpoint lookup of the record and of the
    prefix (e.l + 1) run in 64 bits."""
    import torch
    length = 29
    reads = {"A": 2 * 10 ** 7, "C": 2 * 10 ** 7, "G": 2 * 10 ** 7, "T": 9 * 10 ** 7}
    total = sum(reads.values()) * (length + 1)
    assert total == 45 * 10 ** 8 > 2 ** 32
    if torch.cuda.mem_get_info(0)[0] < 8 * total:
        pytest.skip("needs %.0f GB of free HBM" % (8 * total / 1e9))
    b = msbwt.RleBWT(device=0)
    b.load_vector(homopolymer_rle(reads, length, str(tmp_path / "homopolymers.npy")))
    assert b.get_total_size() == total
    b.set_spectrum_frontier(4096)
    block, at = {}, sum(reads.values())
    for c in "ACGT":
        block[c] = at
        at += reads[c] * length
    for k in (27, 28):
        want = sorted((word_of(c * k), reads[c] * (length - k + 1), block[c] + (k - 1) * reads[c], 0x11 << "ACGT".index(c)) for c in "ACGT")
        assert (max(x[2] for x in want) > 2 ** 32) == (k == 28)
        for min_count, min_edge in ((1, 0), (2 * 10 ** 7, 2 * 10 ** 7)):
            w, c, e, l = b.enumerate_kmer_graph(k, min_count=min_count, min_edge=min_edge or None, ranges=True)
            assert list(zip(w.tolist(), c.tolist(), l.tolist(), e.tolist())) == want, (k, min_count)
            table, nodes, edges = b.kmer_graph_degrees(k, min_count=min_count, min_edge=min_edge or None)
            assert nodes == edges == 4 == table[1, 1] and np.count_nonzero(table) == 1
        # an edge threshold between the counts of the (k+1)-mers: T keeps its loop, the others lose theirs
        w, c, e = b.enumerate_kmer_graph(k, min_count=1, min_edge=reads["A"] * (length - k) + 1)
        assert e.tolist() == [0, 0, 0, 0x88] and w.tolist() == [x[0] for x in want]
