"""Canonical k-mers (csrc/canonical.hip, csrc/spectrum.cpp): the spectrum and the dump with a k-mer and its reverse complement as one class.

Expected values never come from the code under test: the census of tests/test_gpu_spectrum.py (a Counter, or np.unique, over the
ACGT-only windows of the reads) is keyed by min(word, rc word) here, with the counts of the two strands kept apart; rc is restated in
numpy field by field.  Closed forms for the hand-made sets, the palindromes and the homopolymers.

Shapes: the ragged sets of the plain spectrum's tests with every second read reverse-complemented; a hand-made set with one class of
each (own, other) shape the emission rule and the pruning bound can get wrong; the 20 000-base genomes' read sets on every index form,
with the automatic frontier and with the smallest one (64 nodes: the staging overflows, chunks are flushed one by one, the root is
re-seeded); one index beyond 2^32 rows.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_merge_many import EMPTY, homopolymer_rle
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_spectrum import KS, WINDOWS, census_of_matrix, census_of_texts, loaded, word_of

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
COMPLEMENT = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)  # $ A C G N T -> $ T G C N A


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def rc_text(read):
    return read[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rc_words(words, k):
    """packed reverse complements, restated: field by field"""
    w = np.asarray(words, dtype=U64)
    out = np.zeros(len(w), dtype=U64)
    for j in range(k):  # field j (from the low end) becomes field k - 1 - j, complemented
        out |= (U64(3) - ((w >> U64(2 * j)) & U64(3))) << U64(2 * (k - 1 - j))
    return out


def canonical_census(words, counts, k):
    """the plain census (words, counts) -> (canonical words ascending, own, other)"""
    rcw = rc_words(words, k)
    canonical = words <= rcw
    cw, inverse = np.unique(np.where(canonical, words, rcw), return_inverse=True)
    own, other = np.zeros(len(cw), dtype=U64), np.zeros(len(cw), dtype=U64)
    np.add.at(own, inverse[canonical], counts[canonical])
    np.add.at(other, inverse[~canonical], counts[~canonical])
    return cw, own, other


def both_strands_texts(reads):
    return [rc_text(r) if i % 2 else r for i, r in enumerate(reads)]


def check_spectrum(b, k, own, other, plain_occurrences, bins=(2, 3, 256)):
    total = own + other
    for nb in bins:
        hist, distinct, occurrences = b.canonical_kmer_spectrum(k, nb)
        want = np.bincount(np.minimum(total, U64(nb - 1)).astype(np.int64), minlength=nb).astype(U64)
        assert hist.dtype == U64 and np.array_equal(hist, want), (k, nb, hist[:8], want[:8])
        assert hist[0] == 0 and distinct == len(total) == int(hist.sum()), (k, nb, distinct)
        assert occurrences == int(total.sum()) == plain_occurrences, (k, nb, occurrences, plain_occurrences)


def check_dump(b, k, cw, own, other):
    w, o, t = b.enumerate_canonical_kmers(k, sorted=True, strands=True)
    assert w.dtype == o.dtype == t.dtype == U64
    assert np.array_equal(w, cw), (k, len(w), len(cw))
    assert np.array_equal(o, own) and np.array_equal(t, other), k
    if k % 2:
        assert not (w == rc_words(w, k)).any()  # no palindrome of odd length
    return w, o, t


def check_all(b, k, cw, own, other):
    check_spectrum(b, k, own, other, b.kmer_spectrum(k)[2])
    check_dump(b, k, cw, own, other)
    total = own + other
    uw, uc = b.enumerate_canonical_kmers(k)  # the order of the walk
    order = np.argsort(uw, kind="stable")
    assert np.array_equal(uw[order], cw) and np.array_equal(uc[order], total), k
    for lo, hi in WINDOWS:
        keep = (total >= lo) & ((total <= hi) if hi else True)
        gw, go, gt = b.enumerate_canonical_kmers(k, min_count=lo, max_count=hi or None, sorted=True, strands=True)
        assert np.array_equal(gw, cw[keep]) and np.array_equal(go, own[keep]) and np.array_equal(gt, other[keep]), (k, lo, hi)
        assert not (lo == 10 ** 9 and len(gw))
    gw, gc = b.enumerate_canonical_kmers(k, min_count=0, sorted=True)  # 0 is 1
    assert np.array_equal(gw, cw) and np.array_equal(gc, total)


# ---- 1. ragged sets, both strands ----

@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets_with_every_second_read_reverse_complemented(orc, seed):
    reads = both_strands_texts(ragged_set(seed))
    assert any("N" in r for r in reads)
    b = loaded(naive_rle(orc, reads))
    for k in KS:
        check_all(b, k, *canonical_census(*census_of_texts(reads, k), k))
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)  # the sinks fed chunk by chunk
    for k in (4, 17, 32):
        cw, own, other = canonical_census(*census_of_texts(reads, k), k)
        check_spectrum(b, k, own, other, int((own + other).sum()), bins=(3, 256))
        info = b.spectrum_info()
        assert info["chunks"] * _lib.SPECTRUM_MIN_FRONTIER >= info["nodes"][k] >= len(cw)  # (a chunk stages a frontier at most)
        check_dump(b, k, cw, own, other)


# ---- 2. the emission rule and the pruning bound ----

def test_one_class_of_every_shape_through_the_windows(orc):
    """Reads exactly k long, so a read is one k-mer: class i is written `own` times as its canonical k-mer and `other` times as the
    reverse complement.  (1, 1) at min_count = 2 is lost by a walk that prunes at the window's minimum (each strand's suffixes are one
    wide); (0, 3) and (1, 2) are lost by an emitter that is always the canonical member (absent, or pruned at ceil(3 / 2) = 2)."""
    k = 13
    rng = np.random.default_rng(2024)
    shapes = [(1, 1), (2, 1), (1, 2), (3, 0), (0, 3), (2, 2)]
    names, reads = {}, []
    while len(names) < len(shapes):
        q = "".join(rng.choice(list("ACGT"), size=k))
        w = min(q, rc_text(q))
        if w == rc_text(w) or w in names.values():
            continue
        shape = shapes[len(names)]
        names[shape] = w
        reads += [w] * shape[0] + [rc_text(w)] * shape[1]
    rng.shuffle(reads)
    reads = [str(r) for r in reads]
    cw, own, other = canonical_census(*census_of_texts(reads, k), k)
    assert sorted(zip(cw.tolist(), own.tolist(), other.tolist())) == sorted((word_of(w), s[0], s[1]) for s, w in names.items())  # (the census agrees)
    must = {(2, 0): shapes, (3, 0): [(2, 1), (1, 2), (3, 0), (0, 3), (2, 2)], (4, 0): [(2, 2)], (5, 0): [], (1, 2): [(1, 1)], (1, 0): shapes, (2, 2): [(1, 1)],
            (3, 3): [(2, 1), (1, 2), (3, 0), (0, 3)], (4, 4): [(2, 2)]}
    for form in (dict(), dict(pair_index=0), dict(block_format="runs")):
        b = loaded(naive_rle(orc, reads), **form)
        for (lo, hi), back in must.items():
            w, o, t = b.enumerate_canonical_kmers(k, min_count=lo, max_count=hi or None, strands=True)
            got = {int(x): (int(y), int(z)) for x, y, z in zip(w, o, t)}
            assert len(got) == len(w) == len(back), (form, lo, hi, got)
            for shape in shapes:
                word = word_of(names[shape])
                if shape in back:
                    assert got.get(word) == shape, (form, lo, hi, shape, names[shape], got.get(word))
                else:
                    assert word not in got, (form, lo, hi, shape, names[shape])
            assert b.enumerate_canonical_kmers_device(k, None, None, None, 0, min_count=lo, max_count=hi or None) == len(back)
        hist, classes, occurrences = b.canonical_kmer_spectrum(k, 8)
        assert hist.tolist() == [0, 0, 1, 4, 1, 0, 0, 0] and classes == 6 and occurrences == 18


# ---- 3. palindromes and single-strand extremes: closed forms ----

def test_palindromes_are_counted_once(orc):
    n = 3
    b = loaded(naive_rle(orc, ["ACGT" * 5] * n))
    closed = {2: {"AC": (5 * n, 5 * n), "CG": (5 * n, 0), "TA": (4 * n, 0)},  # rc(AC) = GT; CG, TA are palindromes
              4: {"ACGT": (5 * n, 0), "CGTA": (4 * n, 4 * n), "GTAC": (4 * n, 0)},  # rc(CGTA) = TACG
              8: {"ACGTACGT": (4 * n, 0), "CGTACGTA": (3 * n, 3 * n), "GTACGTAC": (3 * n, 0)}}
    for k, classes in closed.items():
        assert all(q <= rc_text(q) and (t == 0) == (q == rc_text(q)) for q, (o, t) in classes.items())
        want = sorted((word_of(q), o, t) for q, (o, t) in classes.items())
        w, o, t = b.enumerate_canonical_kmers(k, sorted=True, strands=True)
        assert list(zip(w.tolist(), o.tolist(), t.tolist())) == want, k
        hist, distinct, occurrences = b.canonical_kmer_spectrum(k, 64)
        assert distinct == 3 and occurrences == n * (20 - k + 1) == b.kmer_spectrum(k)[2]
        assert hist.tolist() == np.bincount([o + t for _, o, t in want], minlength=64).tolist()
    # every palindrome of length 2 (AT, CG, GC, TA) beside non-palindromes, by the census
    reads = ["ACGT" * 5, "GCAT" * 5, "ATAT", "GGCC"]
    b = loaded(naive_rle(orc, reads))
    for k in (2, 4, 8):
        cw, own, other = canonical_census(*census_of_texts(reads, k), k)
        w, o, t = check_dump(b, k, cw, own, other)
        pal = w == rc_words(w, k)
        assert pal.sum() >= 2 and not t[pal].any() and t[~pal].any()
        if k == 2:
            assert {word_of(q) for q in ("AT", "CG", "GC", "TA")} <= set(w[pal].tolist())


def test_a_class_is_found_from_whichever_strand_the_index_holds(orc):
    copies, length = 7, 30
    only_a, only_t = loaded(naive_rle(orc, ["A" * length] * copies)), loaded(naive_rle(orc, ["T" * length] * copies))
    for k in (1, 2, 5, 30):
        c = copies * (length - k + 1)
        w, o, t = only_a.enumerate_canonical_kmers(k, strands=True)
        assert (w.tolist(), o.tolist(), t.tolist()) == ([0], [c], [0]), k
        w, o, t = only_t.enumerate_canonical_kmers(k, strands=True)  # emitted from the non-canonical member T^k: A^k is absent
        assert (w.tolist(), o.tolist(), t.tolist()) == ([0], [0], [c]), k
        for b in (only_a, only_t):
            assert b.enumerate_canonical_kmers(k, min_count=c, max_count=c)[1].tolist() == [c]
            assert b.enumerate_canonical_kmers(k, min_count=c + 1)[0].size == 0
            hist, distinct, occurrences = b.canonical_kmer_spectrum(k, c + 2)
            assert hist[c] == 1 and hist.sum() == 1 and distinct == 1 and occurrences == c
    assert only_a.enumerate_canonical_kmers(31)[0].size == 0


# ---- 4. read sets with errors, every index form; 5. against the library's own verified calls ----

FORMS = {"defaults": dict(), "no pair index": dict(pair_index=0), "pair stride 96": dict(pair_index=1, pair_stride=96), "run blocks": dict(block_format="runs"),
         "sparse table 16": dict(sparse_table=16)}
_sets = {}


def both_strands_set(name):
    """(rle built by the library from read_set(name) with every second read reverse-complemented, its reads as a matrix)"""
    if name not in _sets:
        (flat, offsets), _ = read_set(name)
        reads = flat.reshape(-1, int(offsets[1])).copy()
        reads[1::2] = COMPLEMENT[reads[1::2, ::-1]]
        rle = msbwt.RleBWT(device=0).build_from_reads((reads.reshape(-1), offsets))
        _sets[name] = (rle, reads, {})
    return _sets[name]


def both_strands_census(name, k):
    rle, reads, cache = both_strands_set(name)
    if k not in cache:
        cache[k] = canonical_census(*census_of_matrix(reads, k), k)
    return cache[k]


def walked(b, k, sparse):
    """the dump in the order of the walk, the solid classes and the spectrum of one handle state, and what the dump's writing walk did"""
    if sparse:
        b.set_search_counters(True)
        b.search_counters()
    dump = b.enumerate_canonical_kmers(k, strands=True)
    if sparse:  # the other strand's search looked its queries up in the sparse table
        cnt = b.search_counters()
        b.set_search_counters(False)
        assert cnt["table_steps"] > 0 and cnt["searched"] > 0, cnt
    info = b.spectrum_info()
    return dump, b.enumerate_canonical_kmers(k, min_count=2, strands=True), b.canonical_kmer_spectrum(k), info


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("name", ["plain_100", "repeat_150"])
def test_read_sets_on_every_index_form_and_frontier(name, k, form):
    """Every form against the census, so all forms give identical records.  With the frontier at its minimum of 64 nodes the staging
    overflows (retries), the sinks are fed chunk by chunk, and a walk from the root re-seeds (descents).  A walk seeded from a flat
    direct table (no pair index, run blocks: 4^9 seeds) never meets a single seed whose subtree does not fit, so those forms only
    count under the cap as they are and run the capped dump without their table, from the root.  The capped dump is the device form
    with a capacity known to suffice (two walks, not the three of the two-call pattern), and the capped spectrum is left to
    test_ragged_sets_with_every_second_read_reverse_complemented: on an MI355X a capped walk of plain_100 at k = 21 takes 0.41 s
    (3583 chunks, 758 retries, 273 descents from the root; 4063 chunks, 34 retries from the flat table; twice that on run blocks)
    against 0.5 ms for a whole dump with the automatic frontier; the slowest case, run blocks at k = 31, takes 5 s."""
    import torch
    rle, reads, _ = both_strands_set(name)
    cw, own, other = both_strands_census(name, k)
    total = own + other
    keep = total >= 2
    assert len(cw) > 10 ** 4 and (other > 0).sum() > 100 and (own == 0).sum() > 100 and ((own == 1) & (other == 1)).sum() >= 1
    knobs, sparse = FORMS[form], form == "sparse table 16"
    b = msbwt.RleBWT(device=0)
    if "block_format" in knobs:
        b.set_block_format(knobs["block_format"])
    if sparse:
        b.set_query_length(k)
    b.load_vector(rle)
    for knob in ("pair_index", "pair_stride", "sparse_table"):
        if knob in knobs:
            getattr(b, "set_" + knob)(knobs[knob])
    if sparse:
        assert b.get_sparse_table() == 16 and b.get_query_length() == k

    def same_records(got, want, why):
        order = np.argsort(got[0], kind="stable")
        assert all(np.array_equal(g[order], w) for g, w in zip(got, want)), why

    def report(frontier, info, classes):
        print("%s k = %d, %s, frontier %d: seed depth %d, %d chunks, %d retries, %d descents, %d k-mers staged, %d classes, %.1f ms"
              % (name, k, form, frontier, info["seed_depth"], info["chunks"], info["retries"], info["descents"], info["nodes"][k], classes, info["ms"]))
        assert info["k"] == k and len(cw) <= info["nodes"][k] <= 2 * len(cw)
        return info

    # the automatic frontier
    dump, solid, spectrum, info = walked(b, k, sparse)
    report(0, info, len(dump[0]))
    same_records(dump, (cw, own, other), form)
    same_records(solid, (cw[keep], own[keep], other[keep]), form)
    want_hist = np.bincount(np.minimum(total, U64(255)).astype(np.int64), minlength=256).astype(U64)
    assert np.array_equal(spectrum[0], want_hist) and spectrum[1:] == (len(cw), int(total.sum())), form
    assert info["retries"] == 0 and info["descents"] == 0
    # the smallest frontier
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)
    if info["seed_depth"]:  # seeded from the flat table: counted as it is, then everything else from the root
        assert form in ("no pair index", "run blocks")
        assert b.enumerate_canonical_kmers_device(k, None, None, None, 0) == len(cw)
        capped = report(_lib.SPECTRUM_MIN_FRONTIER, b.spectrum_info(), len(cw))
        assert capped["seed_depth"] == info["seed_depth"] and capped["chunks"] > 1 and capped["retries"] > 0 and capped["descents"] == 0, (form, capped)
        b.set_table_depth(0)
    bufs = [torch.empty(len(cw), dtype=torch.int64, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    assert b.enumerate_canonical_kmers_device(k, *[x.data_ptr() for x in bufs], len(cw)) == len(cw)
    b.device_status(0)
    capped = report(_lib.SPECTRUM_MIN_FRONTIER, b.spectrum_info(), len(cw))
    assert capped["seed_depth"] == 0 and capped["chunks"] > 1 and capped["retries"] > 0 and capped["descents"] > 0, (form, capped)
    same_records(tuple(x.cpu().numpy().astype(U64) for x in bufs), (cw, own, other), (form, "capped"))
    b.set_spectrum_frontier(0)
    if form in ("defaults", "run blocks"):  # ---- 5. the library's own verified calls
        w, o, t = dump
        rcw = rc_words(w, k)
        pal = w == rcw
        assert np.array_equal(msbwt.rle_bwt.reverse_complement_2bit(w, k), rcw)
        assert np.array_equal(b.count_kmers_packed(w, k), o)
        assert np.array_equal(b.count_kmers_packed(rcw, k)[~pal], t[~pal]) and not t[pal].any()
        pw, pc = b.enumerate_kmers(k, sorted=True)
        prc = rc_words(pw, k)
        palindromes, unpaired = int((pw == prc).sum()), int((~np.isin(prc, pw)).sum())
        assert (len(pw) + palindromes + unpaired) % 2 == 0 and len(w) == (len(pw) + palindromes + unpaired) // 2
        assert int(pc.sum()) == int((o + t).sum())
        assert palindromes == 0 or k % 2 == 0


# ---- 6. capacity pattern and empties ----

def test_capacity_pattern_of_both_forms(orc):
    import torch
    dev = torch.device("cuda:0")
    name, k = "plain_100", 17
    rle, _, _ = both_strands_set(name)
    cw, own, other = both_strands_census(name, k)
    keep = own + other >= 2
    n = int(keep.sum())
    b = loaded(rle)
    stream = torch.cuda.current_stream(dev).cuda_stream
    before = b.device_bytes()
    assert b.enumerate_canonical_kmers_device(k, None, None, None, 0, min_count=2, stream=stream) == n > 100
    bufs = [torch.full((n + 3,), -7, dtype=torch.int64, device=dev) for _ in range(3)]
    ptrs = [t.data_ptr() for t in bufs]
    with pytest.raises(MsbwtError) as err:
        b.enumerate_canonical_kmers_device(k, *ptrs, n - 1, min_count=2, stream=stream)
    assert err.value.code == _lib.ERR_INVALID_ARG and err.value.n == n and str(n) in str(err.value)
    assert all(bool((t == -7).all()) for t in bufs)  # nothing written
    assert b.enumerate_canonical_kmers_device(k, *ptrs, n, min_count=2, stream=stream) == n
    b.device_status(stream)
    got = [t.cpu().numpy() for t in bufs]
    assert all((g[n:] == -7).all() for g in got)  # exactly n
    w, o, t = (g[:n].astype(U64) for g in got)
    order = np.argsort(w, kind="stable")
    assert np.array_equal(w[order], cw[keep]) and np.array_equal(o[order], own[keep]) and np.array_equal(t[order], other[keep])
    only = torch.full((n,), -7, dtype=torch.int64, device=dev)  # own and other are optional
    assert b.enumerate_canonical_kmers_device(k, only.data_ptr(), None, None, n, min_count=2, stream=stream) == n
    assert np.array_equal(np.sort(only.cpu().numpy().astype(U64)), cw[keep])
    b.device_status(stream)
    # the host form
    lib, count = _lib.lib(), C.c_uint64(0)
    host = [np.full(n, 7, dtype=U64) for _ in range(3)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, k, 2, 0, ptr(host[0]), ptr(host[1]), ptr(host[2]), n - 1, C.byref(count)) == _lib.ERR_INVALID_ARG
    assert count.value == n and str(n).encode() in lib.msbwt_rle_last_error(b._h) and all((a == 7).all() for a in host)
    assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, k, 2, 0, ptr(host[0]), None, ptr(host[2]), n, C.byref(count)) == 0 and count.value == n
    order = np.argsort(host[0], kind="stable")
    assert np.array_equal(host[0][order], cw[keep]) and (host[1] == 7).all() and np.array_equal(host[2][order], other[keep])
    assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, k, 2, 0, None, None, None, 5, C.byref(count)) == _lib.ERR_INVALID_ARG  # a capacity and no buffer
    assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, k, 5, 2, None, None, None, 0, C.byref(count)) == _lib.ERR_INVALID_ARG
    for bad in (0, 33):
        assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, bad, 1, 0, None, None, None, 0, C.byref(count)) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_canonical_kmer_spectrum(b._h, bad, ptr(host[0]), 8, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_canonical_kmer_spectrum(b._h, 3, ptr(host[0]), 1, None, None) == _lib.ERR_INVALID_ARG
    assert b.device_bytes() == before


@pytest.mark.parametrize("name", ["empty index", "empty reads", "N only"])
def test_indexes_without_a_kmer(orc, name):
    reads = {"empty index": [], "empty reads": [""] * 7, "N only": ["NNNN", "N", "NN"]}[name]
    b = loaded(naive_rle(orc, reads) if reads else EMPTY)
    for k in (1, 2, 5, 31, 32):
        hist, distinct, occurrences = b.canonical_kmer_spectrum(k)
        assert not hist.any() and distinct == 0 and occurrences == 0
        assert all(a.size == 0 for a in b.enumerate_canonical_kmers(k, strands=True))
        assert b.enumerate_canonical_kmers_device(k, None, None, None, 0) == 0


# ---- 7. beyond 2^32 rows ----

def test_beyond_2_to_32_rows(tmp_path):
    """Homopolymer reads (test_gpu_merge_many.homopolymer_rle), 4.5e9 rows, of A and a few of T: the class A^k is written n_A (length - k + 1)
    times as itself -- more than 2^32 at k = 1 -- and n_T (length - k + 1) times as T^k."""
    import torch
    length = 29
    reads = {"A": 149 * 10 ** 6, "T": 10 ** 6}
    total = sum(reads.values()) * (length + 1)
    assert total == 45 * 10 ** 8 > 2 ** 32
    if torch.cuda.mem_get_info(0)[0] < 8 * total:
        pytest.skip("needs %.0f GB of free HBM" % (8 * total / 1e9))
    b = msbwt.RleBWT(device=0)
    b.load_vector(homopolymer_rle(reads, length, str(tmp_path / "homopolymers.npy")))
    assert b.get_total_size() == total
    b.set_spectrum_frontier(4096)
    for k in (1, 2, 29):
        own, other = reads["A"] * (length - k + 1), reads["T"] * (length - k + 1)
        assert (own > 2 ** 32) == (k == 1)
        w, o, t = b.enumerate_canonical_kmers(k, strands=True)
        assert (w.tolist(), o.tolist(), t.tolist()) == ([0], [own], [other]), k
        assert b.enumerate_canonical_kmers(k, min_count=own + other, max_count=own + other)[1].tolist() == [own + other]
        assert b.enumerate_canonical_kmers(k, min_count=own + other + 1)[0].size == 0
        hist, distinct, occurrences = b.canonical_kmer_spectrum(k, 4)
        assert hist.tolist() == [0, 0, 0, 1] and distinct == 1 and occurrences == own + other == b.kmer_spectrum(k, 4)[2]
    assert b.enumerate_canonical_kmers(30)[0].size == 0
