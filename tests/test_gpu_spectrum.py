"""The k-mers an index holds (csrc/spectrum.hip, csrc/spectrum.cpp): abundance spectrum and k-mer dump.

Expected values never come from the code under test: a Counter over the ACGT-only windows of the reads (for the 4000-read sets the
same census by numpy: np.unique over the windows' 2-bit words), the CPU oracle's constrain_range for every range start, and closed
forms for homopolymer reads.

Shapes: ragged sets of 1-50 reads of 0-70 symbols with N, duplicates and prefixes; the 20 000-base genome's read sets with 0.5 %
errors (4.0e5 symbols); k at both parities, around 16 and at the single-word limit 30, 31, 32; a frontier cap at its minimum, which
on those read sets means thousands of chunks, retries and -- from the root -- re-seeding; every index form (the default one has a
packed direct table, so its walks start at the root; without a pair index and on run blocks the table stays flat and seeds the
walks of k > 9); one index beyond 2^32 rows.  Run with `pytest -m gpu`."""
import importlib
import os
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from test_gpu_merge_many import EMPTY, homopolymer_rle
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_sparse import oracle_ranges

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
pack_2bit, unpack_2bit = msbwt.rle_bwt.pack_2bit, msbwt.rle_bwt.unpack_2bit
U64 = np.uint64
KS = (1, 2, 3, 4, 15, 16, 17, 30, 31, 32)
WINDOWS = ((2, 0), (1, 1), (3, 7), (10 ** 9, 0))  # (min_count, max_count); the last matches nothing


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def word_of(kmer):
    w = 0
    for c in kmer:
        w = w << 2 | "ACGT".index(c)
    return w


def census_of_texts(reads, k):
    """(sorted words, their counts) of the ACGT-only windows of length k of reads given as strings: a Counter."""
    c = Counter(r[i:i + k] for r in reads for i in range(len(r) - k + 1) if set(r[i:i + k]) <= set("ACGT"))
    pairs = sorted((word_of(q), n) for q, n in c.items())
    return np.array([p[0] for p in pairs], dtype=U64), np.array([p[1] for p in pairs], dtype=U64)


def census_of_matrix(reads, k):
    """the same for an (n, length) matrix of symbol codes, by numpy"""
    code = np.full(6, 255, dtype=np.uint8)
    code[[1, 2, 3, 5]] = [0, 1, 2, 3]
    if reads.shape[1] < k:
        return np.zeros(0, dtype=U64), np.zeros(0, dtype=U64)
    win = np.lib.stride_tricks.sliding_window_view(code[reads], k, axis=1).reshape(-1, k)
    win = win[(win != 255).all(axis=1)].astype(U64)
    words = np.zeros(len(win), dtype=U64)
    for j in range(k):
        words = (words << U64(2)) | win[:, j]
    words, counts = np.unique(words, return_counts=True)
    return words, counts.astype(U64)


_census = {}


def read_set_census(name, k):
    if (name, k) not in _census:
        (flat, offsets), _ = read_set(name)
        length = int(offsets[1])
        _census[name, k] = census_of_matrix(flat.reshape(-1, length), k)
    return _census[name, k]


def loaded(rle, **knobs):
    """RleBWT with `rle` loaded; knobs: block_format (before the load); pair_index, pair_stride, table_depth, sparse_table (after)."""
    b = msbwt.RleBWT(device=0)
    if "block_format" in knobs:
        b.set_block_format(knobs["block_format"])
    b.load_vector(rle)
    for name in ("pair_index", "pair_stride", "table_depth", "sparse_table"):
        if name in knobs:
            getattr(b, "set_" + name)(knobs[name])
    return b


def oracle_of(orc, rle):
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    return ref


def check_spectrum(b, k, words, counts, bins=(2, 3, 256)):
    for nb in bins:
        hist, distinct, occurrences = b.kmer_spectrum(k, nb)
        want = np.bincount(np.minimum(counts, U64(nb - 1)).astype(np.int64), minlength=nb).astype(U64)
        assert hist.dtype == U64 and np.array_equal(hist, want), (k, nb, hist[:8], want[:8])
        assert hist[0] == 0 and distinct == len(words) == int(hist.sum()) and occurrences == int(counts.sum()), (k, nb, distinct, occurrences)


def check_sorted_dump(b, ref, k, words, counts):
    w, c, l = b.enumerate_kmers(k, sorted=True, ranges=True)
    assert w.dtype == c.dtype == l.dtype == U64
    assert np.array_equal(w, words), (k, len(w), len(words))
    assert np.array_equal(c, counts), k
    if len(w):
        ol, oh = oracle_ranges(ref, unpack_2bit(words, k))
        assert np.array_equal(oh - ol, counts), k  # (the oracle agrees with the census)
        assert np.array_equal(l, ol), (k, np.flatnonzero(l != ol)[:5])
        assert np.all(l[1:] > l[:-1]) and np.all(l[1:] >= (l + c)[:-1]), k
    return w, c, l


def check_all(b, ref, k, words, counts):
    check_spectrum(b, k, words, counts)
    w, c, _ = check_sorted_dump(b, ref, k, words, counts)
    uw, uc = b.enumerate_kmers(k, sorted=False)
    order = np.argsort(uw, kind="stable")
    assert np.array_equal(uw[order], words) and np.array_equal(uc[order], counts), k
    for lo, hi in WINDOWS:
        keep = (counts >= lo) & ((counts <= hi) if hi else True)
        gw, gc = b.enumerate_kmers(k, min_count=lo, max_count=hi or None)
        assert np.array_equal(gw, words[keep]) and np.array_equal(gc, counts[keep]), (k, lo, hi)
        assert not (lo == 10 ** 9 and len(gw))
    gw, gc = b.enumerate_kmers(k, min_count=0)  # 0 is 1
    assert np.array_equal(gw, words)
    if len(w) and b.get_block_format() == "planes":
        assert np.array_equal(b.count_kmers_packed(w, k), c), k


# ---- 1. exactness on small sets ----

@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets_at_every_k(orc, seed):
    reads = ragged_set(seed)
    rle = naive_rle(orc, reads)
    b, ref = loaded(rle), oracle_of(orc, rle)
    for k in KS:
        check_all(b, ref, k, *census_of_texts(reads, k))


@pytest.mark.parametrize("k", KS)
def test_read_set_with_errors(orc, k):
    _, rle = read_set("plain_100")
    words, counts = read_set_census("plain_100", k)
    assert len(words) > (3 if k == 1 else 15) and counts.max() > 1
    check_all(loaded(rle), oracle_of(orc, rle), k, words, counts)


def test_k_longer_than_every_read(orc):
    reads = ["ACGTA", "ACG", "", "TTTTT", "GN"]
    rle = naive_rle(orc, reads)
    b, ref = loaded(rle), oracle_of(orc, rle)
    for k in (6, 7, 16, 32):
        hist, distinct, occurrences = b.kmer_spectrum(k)
        assert not hist.any() and distinct == 0 and occurrences == 0
        for srt in (True, False):
            w, c, l = b.enumerate_kmers(k, sorted=srt, ranges=True)
            assert w.size == c.size == l.size == 0
    check_all(b, ref, 5, *census_of_texts(reads, 5))


# ---- 2. degenerate indexes ----

@pytest.mark.parametrize("name", ["empty reads", "G", "N only", "two_string", "empty index"])
def test_degenerate_indexes(orc, name):
    reads = {"empty reads": [""] * 7, "G": ["G"], "N only": ["NNNN", "N", "NN"], "two_string": None, "empty index": []}[name]
    if name == "two_string":
        rle = np.array(np.load(os.path.join(GOLDEN_DIR, "two_string.npy")))
        reads = [str(line.strip()) for line in open(os.path.join(GOLDEN_DIR, "two_string.fa")) if not line.startswith(">")]
        assert sum(len(r) + 1 for r in reads) == msbwt.rle_bwt.rle_total(rle) == 10
    else:
        rle = naive_rle(orc, reads) if reads else EMPTY
    b, ref = loaded(rle), oracle_of(orc, rle)
    for k in (1, 2, 3, 4, 5, 31, 32):
        words, counts = census_of_texts(reads, k)
        assert name in ("G", "two_string") or len(words) == 0
        check_all(b, ref, k, words, counts)
    assert b.kmer_spectrum(1)[1] == {"G": 1, "two_string": 4}.get(name, 0)


# ---- 3. wide ranges: far above the sparse table's escape width 255 and the LDS bins of the histogram ----

def test_wide_ranges_of_a_homopolymer():
    copies, length = 300, 1000
    rng = np.random.default_rng(17)
    others = ["".join(rng.choice(list("ACGTN"), size=int(rng.integers(20, 90)), p=[0.3, 0.2, 0.2, 0.25, 0.05])) for _ in range(60)]
    reads = ["A" * length] * copies + others
    b = msbwt.RleBWT(device=0)
    b.load_reads(reads, ascii=True)
    for k in (4, 21):
        small = Counter(r[i:i + k] for r in others for i in range(len(r) - k + 1) if set(r[i:i + k]) <= set("ACGT"))
        top = copies * (length - k + 1) + small.get("A" * k, 0)  # the closed form
        assert top > 2048 * 100
        small["A" * k] = top
        pairs = sorted((word_of(q), n) for q, n in small.items())
        words, counts = np.array([p[0] for p in pairs], dtype=U64), np.array([p[1] for p in pairs], dtype=U64)
        assert words[0] == 0 and counts[0] == top
        check_spectrum(b, k, words, counts, bins=(top + 2, top + 1, top, 2049, 2048, 256, 2))
        hist = b.kmer_spectrum(k, top + 2)[0]
        assert hist[top] == 1 and hist[top + 1] == 0
        assert b.kmer_spectrum(k, 256)[0][255] == int((counts >= 255).sum()) >= 1
        w, c, l = b.enumerate_kmers(k, ranges=True)
        assert np.array_equal(w, words) and np.array_equal(c, counts)
        w, c = b.enumerate_kmers(k, min_count=top, max_count=top, sorted=False)
        assert w.tolist() == [0] and c.tolist() == [top]


# ---- 4. chunking ----

def info_after(b, call):
    out = call()
    return out, b.spectrum_info()


@pytest.mark.parametrize("seeds", ["root", "flat table"])
def test_a_frontier_at_its_minimum_gives_the_same_results(orc, seeds):
    """read_set("plain_100") at k = 31 with the frontier capped to MSBWT_SPECTRUM_MIN_FRONTIER = 64 nodes.  From the root (the default
    index's direct table is packed, which is no seed source) the only seed's subtree never fits: the walk re-seeds level by level.
    From the flat direct table an index without a pair index keeps (9 symbols deep here) the seeds are its 4^9 entries, first 65 536
    at a time: chunks taken again at half size.  Seen on an MI355X on this input: from the root 3067 chunks, 673 retries, 273
    descents, 0.38 s per walk against 0.4 ms with the automatic frontier."""
    _, rle = read_set("plain_100")
    k = 31
    words, counts = read_set_census("plain_100", k)
    b = loaded(rle) if seeds == "root" else loaded(rle, pair_index=0)
    auto_spec, auto_info = info_after(b, lambda: b.kmer_spectrum(k))
    auto_dump = b.enumerate_kmers(k, ranges=True)
    auto_loose = b.enumerate_kmers(k, sorted=False, min_count=2)
    assert auto_info["k"] == k and auto_info["retries"] == 0 and auto_info["descents"] == 0 and auto_info["chunks"] >= 1
    assert auto_info["nodes"][k] == len(words) and (auto_info["seed_depth"] == 0) == (seeds == "root")
    with pytest.raises(MsbwtError) as err:
        b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER - 1)
    assert err.value.code == _lib.ERR_INVALID_ARG
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)
    spec, info = info_after(b, lambda: b.kmer_spectrum(k))
    print("frontier %d, seeds: %s: seed depth %d, %d chunks, %d retries, %d descents, %.1f ms (automatic: %d chunks, %.1f ms)"
          % (_lib.SPECTRUM_MIN_FRONTIER, seeds, info["seed_depth"], info["chunks"], info["retries"], info["descents"], info["ms"],
             auto_info["chunks"], auto_info["ms"]))
    assert np.array_equal(spec[0], auto_spec[0]) and spec[1:] == auto_spec[1:] == (len(words), int(counts.sum()))
    assert info["chunks"] > 1 and info["retries"] >= 1 and info["seed_depth"] == auto_info["seed_depth"]
    assert np.array_equal(info["nodes"], auto_info["nodes"])
    if seeds == "root":
        assert info["descents"] >= 1
    dump = b.enumerate_kmers(k, ranges=True)
    assert all(np.array_equal(x, y) for x, y in zip(dump, auto_dump)) and np.array_equal(dump[0], words) and np.array_equal(dump[1], counts)
    loose = b.enumerate_kmers(k, sorted=False, min_count=2)
    assert sorted(zip(loose[0].tolist(), loose[1].tolist())) == sorted(zip(auto_loose[0].tolist(), auto_loose[1].tolist()))
    b.set_spectrum_frontier(0)
    assert b.spectrum_info()["k"] == k and info_after(b, lambda: b.kmer_spectrum(k))[1]["retries"] == 0


# ---- 5. every index form gives the same answer ----

FORMS = {"pair stride 96": dict(pair_index=1, pair_stride=96), "pair stride 128": dict(pair_index=1, pair_stride=128), "no pair index": dict(pair_index=0),
         "run blocks": dict(block_format="runs"), "no direct table": dict(table_depth=0), "no sparse table": dict(sparse_table=0), "sparse table 16": dict(sparse_table=16),
         "defaults": dict()}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_index_form_gives_the_same_answer(orc, form):
    _, rle = read_set("repeat_100")
    knobs = FORMS[form]
    b, ref = loaded(rle, **knobs), oracle_of(orc, rle)
    assert b.get_block_format() == knobs.get("block_format", "planes")
    if "pair_index" in knobs:
        assert b.get_pair_index() == bool(knobs["pair_index"])
    if "pair_stride" in knobs:
        assert b.get_pair_stride() == knobs["pair_stride"]
    if "table_depth" in knobs:
        assert b.get_table_depth() == 0
    if "sparse_table" in knobs:
        assert b.get_sparse_table() == knobs["sparse_table"]
    if form == "run blocks":
        assert not b.get_pair_index()
    for k in (5, 16, 31):
        words, counts = read_set_census("repeat_100", k)
        check_spectrum(b, k, words, counts, bins=(256,))
        check_sorted_dump(b, ref, k, words, counts)
        print("%s, k = %d: seed depth %d" % (form, k, b.spectrum_info()["seed_depth"]))


# ---- 6. the builder's own census ----

def test_the_sparse_builders_census_is_the_spectrums():
    _, rle = read_set("plain_150")
    b = loaded(rle, pair_index=1, sparse_table=21)
    info = b.sparse_table_info()
    assert info["depth"] == 21 and len(info["distinct"]) >= 3
    compared = 0
    for d, distinct in info["distinct"].items():
        hist, got, _ = b.kmer_spectrum(d)
        assert got == distinct, d
        if info["once"][d]:
            assert hist[1] == info["once"][d], d
            compared += 1
    assert compared >= 2


# ---- 7. pruning ----

def test_a_count_window_prunes_the_walk():
    _, rle = read_set("plain_100")
    k = 31
    words, counts = read_set_census("plain_100", k)
    b = loaded(rle)
    all_of_them, everything = info_after(b, lambda: b.enumerate_kmers(k))
    solid, pruned = info_after(b, lambda: b.enumerate_kmers(k, min_count=2))
    assert np.array_equal(all_of_them[0], words) and np.array_equal(solid[0], words[counts >= 2]) and np.array_equal(solid[1], counts[counts >= 2])
    assert 0 < len(solid[0]) < len(words)
    deep = [d for d in range(k - 8, k + 1) if everything["nodes"][d]]
    assert len(deep) >= 4 and all(pruned["nodes"][d] < everything["nodes"][d] for d in deep), (pruned["nodes"], everything["nodes"])
    assert pruned["nodes"][k] == len(solid[0]) and everything["nodes"][k] == len(words)


# ---- 8. by source without a search ----

def test_the_dumps_ranges_give_the_counts_by_source(orc):
    sets = [ragged_set(21), ragged_set(22) + ["ACGTACGTTTGACC"] * 3, ragged_set(23)]
    b = msbwt.RleBWT(device=0)
    b.load_merged_many([naive_rle(orc, s) for s in sets], keep_sources=True)
    assert b.source_count() == 3
    for k in (3, 8, 21):
        w, c, l = b.enumerate_kmers(k, ranges=True)
        words, counts = census_of_texts(sum(sets, []), k)
        assert np.array_equal(w, words) and np.array_equal(c, counts) and len(w) > 10
        by_range = b.range_sources(l, l + c)
        assert np.array_equal(by_range, b.count_kmers_by_source(unpack_2bit(w, k)))
        for i, s in enumerate(sets):
            own = dict(zip(*(x.tolist() for x in census_of_texts(s, k))))
            assert by_range[:, i].tolist() == [own.get(q, 0) for q in w.tolist()], (k, i)
        assert np.array_equal(by_range.sum(axis=1), c)


# ---- 9. beyond 2^32 rows ----

def test_beyond_2_to_32_rows(tmp_path):
    """Homopolymer reads (test_gpu_merge_many.homopolymer_rle), 4.5e9 rows: the k-mers are c^k, count n_c (length - k + 1), and the range
    of c^k starts (k - 1) n_c rows into the block of c.  T's block reaches across row 2^32.  The walk is four nodes per level; the
    automatic frontier on this index is the full 2^27 nodes (6.4 GB per call), taken once -- the other calls run under a cap.  On an
    MI355X: 2.9 s for the closed-form RLE and the load, 0.6 s for the dump with the automatic frontier, 0.01 s for the rest; where this
    test is the first of its process to start torch (the free-memory gate), that start-up adds 11 s before all of it."""
    import time
    import torch
    started = time.perf_counter()
    length = 29
    reads = {"A": 2 * 10 ** 7, "C": 2 * 10 ** 7, "G": 2 * 10 ** 7, "T": 9 * 10 ** 7}
    total = sum(reads.values()) * (length + 1)
    assert total == 45 * 10 ** 8 > 2 ** 32
    if torch.cuda.mem_get_info(0)[0] < 8 * total:
        pytest.skip("needs %.0f GB of free HBM" % (8 * total / 1e9))
    b = msbwt.RleBWT(device=0)
    t0 = time.perf_counter()
    b.load_vector(homopolymer_rle(reads, length, str(tmp_path / "homopolymers.npy")))
    t1 = time.perf_counter()
    assert b.get_total_size() == total
    block, at = {}, sum(reads.values())
    for c in "ACGT":
        block[c] = at
        at += reads[c] * length
    expected = lambda k: sorted((word_of(c * k), reads[c] * (length - k + 1), block[c] + (k - 1) * reads[c]) for c in "ACGT")
    w, c, l = b.enumerate_kmers(29, ranges=True)  # the automatic frontier
    assert list(zip(w.tolist(), c.tolist(), l.tolist())) == expected(29)
    t2 = time.perf_counter()
    b.set_spectrum_frontier(4096)
    for k in (1, 2, 28, 29):
        want = expected(k)
        for srt in (True, False):
            w, c, l = b.enumerate_kmers(k, sorted=srt, ranges=True)
            got = list(zip(w.tolist(), c.tolist(), l.tolist()))
            assert (got if srt else sorted(got)) == want, (k, srt)
        assert (max(x[2] for x in want) > 2 ** 32) == (k >= 28)
        hist, distinct, occurrences = b.kmer_spectrum(k, 4)
        assert hist.tolist() == [0, 0, 0, 4] and distinct == 4 and occurrences == sum(x[1] for x in want)
    assert b.enumerate_kmers(30)[0].size == 0
    print("set-up %.2f s, load %.2f s, automatic dump %.2f s, the rest %.2f s" % (t0 - started, t1 - t0, t2 - t1, time.perf_counter() - t2))


# ---- 10. the device form ----

def test_device_form_fills_exactly_n_records_or_nothing(orc):
    import torch
    dev = torch.device("cuda:0")
    _, rle = read_set("plain_100")
    k = 17
    words, counts = read_set_census("plain_100", k)
    keep = counts >= 2
    n = int(keep.sum())
    b, ref = loaded(rle), oracle_of(orc, rle)
    ol, _ = oracle_ranges(ref, unpack_2bit(words[keep], k))
    stream = torch.cuda.current_stream(dev).cuda_stream
    before = b.device_bytes()
    assert b.enumerate_kmers_device(k, None, None, None, 0, min_count=2, stream=stream) == n > 100
    for srt in (True, False):
        bufs = [torch.full((n + 3,), -7, dtype=torch.int64, device=dev) for _ in range(3)]
        ptrs = [t.data_ptr() for t in bufs]
        with pytest.raises(MsbwtError) as err:
            b.enumerate_kmers_device(k, *ptrs, n - 1, min_count=2, sorted=srt, stream=stream)
        assert err.value.code == _lib.ERR_INVALID_ARG and err.value.n == n and str(n) in str(err.value)
        assert all(bool((t == -7).all()) for t in bufs)
        assert b.enumerate_kmers_device(k, *ptrs, n, min_count=2, sorted=srt, stream=stream) == n
        b.device_status(stream)
        got = [t.cpu().numpy() for t in bufs]
        assert all((g[n:] == -7).all() for g in got)
        w, c, l = (g[:n].astype(U64) for g in got)
        order = np.arange(n) if srt else np.argsort(w, kind="stable")
        assert np.array_equal(w[order], words[keep]) and np.array_equal(c[order], counts[keep]) and np.array_equal(l[order], ol)
        only = torch.full((n,), -7, dtype=torch.int64, device=dev)  # counts and l are optional
        assert b.enumerate_kmers_device(k, only.data_ptr(), None, None, n, min_count=2, sorted=srt, stream=stream) == n
        assert np.array_equal(np.sort(only.cpu().numpy().astype(U64)), words[keep])
    b.device_status(stream)
    assert b.device_bytes() == before


# ---- the argument guards behind "nothing loaded" (tests/test_spectrum_abi.py has the ones before it) ----

def test_argument_guards_on_a_loaded_index():
    import ctypes as C
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = _lib.lib()
    for rle in (EMPTY, np.array(np.load(os.path.join(GOLDEN_DIR, "two_string.npy")))):
        b = loaded(rle)
        before = b.spectrum_info()
        hist, n = np.zeros(8, dtype=U64), C.c_uint64(77)
        for k in (0, 33, 1000):
            assert lib.msbwt_rle_kmer_spectrum(b._h, k, ptr(hist), 8, None, None) == _lib.ERR_INVALID_ARG
            assert lib.msbwt_rle_enumerate_kmers(b._h, k, 1, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
            assert lib.msbwt_rle_enumerate_kmers_device(b._h, k, 1, 0, 1, None, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID_ARG
        for bins in (0, 1):
            assert lib.msbwt_rle_kmer_spectrum(b._h, 3, ptr(hist), bins, None, None) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_kmer_spectrum(b._h, 3, None, 8, None, None) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_enumerate_kmers(b._h, 3, 5, 2, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_enumerate_kmers(b._h, 3, 1, 0, 1, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_enumerate_kmers(b._h, 3, 1, 0, 1, None, None, None, 5, C.byref(n)) == _lib.ERR_INVALID_ARG  # a capacity and no buffer
        assert n.value == 77 and not hist.any() and b.spectrum_info()["ms"] == before["ms"]  # refused before anything ran
        assert lib.msbwt_rle_enumerate_kmers(b._h, 3, 2, 2, 1, None, None, None, 0, C.byref(n)) == 0 and n.value == 0  # min == max is a window
        hist2, distinct, occurrences = b.kmer_spectrum(1, 2)  # the smallest histogram
        assert hist2.tolist() == [0, 4 if len(rle) else 0] and distinct == int(hist2[1]) and occurrences == (8 if len(rle) else 0)
