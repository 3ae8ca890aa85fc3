"""K-mers by source (csrc/source_spectrum.hip, csrc/spectrum.cpp): one abundance spectrum per input of a merged index, and the k-mer
dump filtered by per-source counts.

Expected values never come from the code under test.  The primary oracle is a census per input -- a Counter (for the read sets
np.unique) over the ACGT-only windows of each input's own reads -- joined on the k-mer word into an n x S matrix; for homopolymer inputs
closed forms.  On top of that the identities: row s of the histogram is kmer_spectrum of input s loaded alone, the dump is
enumerate_kmers(ranges=True) + range_sources + a numpy predicate, the counts sum to the plain dump's, sharing sums to the plain distinct.

Shapes: ragged collections of 1, 2, 3, 8, 9, 17 and 32 inputs (a few thousand rows, an empty input and an input of one empty read among
them: 9 is a second batch of eight lanes partly filled, 17 two checkpoint lines); the 4000-read set cut in three (4.0e5 rows, 400
checkpoint blocks) at k = 1 .. 32, whose small k go through the checkpoints and whose large k are counted from their own bytes;
homopolymer inputs that put a k-mer's total exactly at, one below and one above the border between the two counting paths and the
checkpoint block, with ranges starting on and just off 16-byte and block borders; one index beyond 2^32 rows.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_merge_many import EMPTY, homopolymer_rle, ragged_collection
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_spectrum import census_of_matrix, census_of_texts, word_of

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
NO_LIMIT = (1 << 64) - 1


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def join(censuses):
    """[(sorted words, counts)] per input -> (the sorted union of the words, counts[n, S])"""
    words = np.unique(np.concatenate([w for w, _ in censuses] + [np.zeros(0, dtype=U64)]))
    m = np.zeros((len(words), len(censuses)), dtype=U64)
    for s, (w, c) in enumerate(censuses):
        m[np.searchsorted(words, w), s] = c
    return words, m


def census_of_sets(sets, k):
    return join([census_of_texts(s, k) for s in sets])


def passes(m, lo=None, hi=None, min_total=1, max_total=None):
    """The predicate, restated on the census: hi[s] None = no limit, 0 = absent."""
    keep = np.ones(len(m), dtype=bool)
    for s in range(m.shape[1]):
        if lo is not None:
            keep &= m[:, s] >= U64(lo[s])
        if hi is not None and hi[s] is not None:
            keep &= m[:, s] <= U64(hi[s])
    total = m.sum(axis=1, dtype=U64)
    keep &= total >= U64(max(min_total, 1))
    if max_total:
        keep &= total <= U64(max_total)
    return keep


def check_spectrum(b, k, words, m, bins=(2, 3, 256)):
    S = m.shape[1]
    assert b.source_count() == S
    for nb in bins:
        hist, sharing, distinct, occurrences = b.kmer_spectrum_by_source(k, nb)
        want = np.stack([np.bincount(np.minimum(m[:, s], U64(nb - 1)).astype(np.int64), minlength=nb) for s in range(S)]).astype(U64)
        assert hist.dtype == U64 and hist.shape == (S, nb) and np.array_equal(hist, want), (k, nb, np.argwhere(hist != want)[:5])
        held = (m > 0).sum(axis=1)
        assert np.array_equal(sharing, np.bincount(held, minlength=S + 1).astype(U64)) and sharing[0] == 0, (k, nb, sharing)
        assert np.array_equal(distinct, (m > 0).sum(axis=0).astype(U64)) and np.array_equal(distinct, hist[:, 1:].sum(axis=1)), (k, nb)
        assert np.array_equal(occurrences, m.sum(axis=0, dtype=U64)), (k, nb)
        assert (hist.sum(axis=1) == len(words)).all() and int(sharing.sum()) == len(words)
        assert b.spectrum_info()["k"] == k and b.spectrum_info()["nodes"][k] == len(words)


def check_dump(b, k, words, m, lo=None, hi=None, min_total=1, max_total=None):
    """Sorted with ranges, and unsorted: the same records.  Returns the sorted dump."""
    keep = passes(m, lo, hi, min_total, max_total)
    w, c, l = b.enumerate_kmers_by_source(k, lo, hi, min_total, max_total, sorted=True, ranges=True)
    assert w.dtype == c.dtype == l.dtype == U64 and c.shape == (len(w), m.shape[1])
    assert np.array_equal(w, words[keep]), (k, lo, hi, min_total, max_total, len(w), int(keep.sum()))
    assert np.array_equal(c, m[keep]), (k, np.argwhere(c != m[keep])[:5])
    assert np.all(l[1:] >= (l + c.sum(axis=1, dtype=U64))[:-1])  # disjoint ranges in word order
    uw, uc = b.enumerate_kmers_by_source(k, lo, hi, min_total, max_total, sorted=False)
    order = np.argsort(uw, kind="stable")
    assert np.array_equal(uw[order], w) and np.array_equal(uc[order], c), k
    return w, c, l


def check_against_the_composition(b, k, w, c, l, lo=None, hi=None, min_total=1, max_total=None):
    """enumerate_kmers(ranges=True) + range_sources + the numpy predicate: what the call replaces."""
    pw, pc, pl = b.enumerate_kmers(k, ranges=True)
    by_range = b.range_sources(pl, pl + pc) if len(pw) else np.zeros((0, b.source_count()), dtype=U64)
    keep = passes(by_range, lo, hi, min_total, max_total)
    assert np.array_equal(w, pw[keep]) and np.array_equal(c, by_range[keep]) and np.array_equal(l, pl[keep]), k
    assert np.array_equal(by_range.sum(axis=1, dtype=U64), pc)


def merged(rles):
    b = msbwt.RleBWT(device=0)
    b.load_merged_many(rles, keep_sources=True)
    assert b.source_count() == len(rles)
    return b


# ---- 1. source counts ----

def three_sets():
    """Three ragged read sets that share reads: the two longest reads of the first are in all three, six more of it in the last."""
    first = ragged_set(21) + ragged_set(24)
    shared = sorted(first, key=len)[-2:]
    return [first, ragged_set(22) + ["ACGTACGTTTGACC"] * 3 + shared, ragged_set(23) + ragged_set(21)[:6] + shared]


def collection(S):
    if S == 1:
        return [ragged_set(3) + ragged_set(4) + ragged_set(5)]
    if S == 2:
        return three_sets()[:2]
    if S == 3:
        return three_sets()
    sets = ragged_collection(S, 0)  # (of three inputs it leaves one that is not empty)
    assert [] in sets and [""] in sets
    return sets


@pytest.mark.parametrize("S", [1, 2, 3, 8, 9, 17, 32])
def test_source_counts(orc, S):
    sets = collection(S)
    rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
    b = merged(rles)
    before = b.device_bytes()
    wide = False
    for k in (1, 4, 21):
        words, m = census_of_sets(sets, k)
        assert len(words) >= 4 and (S == 1 or (m > 0).sum(axis=1).max() >= 2)
        wide |= bool((m.sum(axis=1) > msbwt.source_narrow_rows()).any())
        check_spectrum(b, k, words, m)
        w, c, l = check_dump(b, k, words, m)
        check_against_the_composition(b, k, w, c, l)
        plain_hist, plain_distinct, plain_occurrences = b.kmer_spectrum(k)
        hist, sharing, distinct, occurrences = b.kmer_spectrum_by_source(k)
        assert int(sharing.sum()) == plain_distinct and int(occurrences.sum()) == plain_occurrences
        if S == 1:  # the plain calls
            assert np.array_equal(hist[0], plain_hist) and sharing.tolist() == [0, plain_distinct]
            pw, pc, pl = b.enumerate_kmers(k, ranges=True)
            assert np.array_equal(w, pw) and np.array_equal(c[:, 0], pc) and np.array_equal(l, pl)
        if S <= 8:  # row s is the spectrum of input s loaded alone
            for s, rle in enumerate(rles):
                alone = msbwt.RleBWT(device=0)
                alone.load_vector(rle)
                own_hist, own_distinct, own_occurrences = alone.kmer_spectrum(k)
                assert np.array_equal(hist[s, 1:], own_hist[1:]) and distinct[s] == own_distinct and occurrences[s] == own_occurrences, (k, s)
    assert wide  # both counting paths ran
    assert b.device_bytes() == before


# ---- 2. k values, on an index of 400 checkpoint blocks ----

_parts = {}


def three_parts():
    """read_set("plain_100") cut in three: (the parts' read matrices, their BWTs from the device builder, the merged index)"""
    if not _parts:
        (flat, offsets), _ = read_set("plain_100")
        n, length = offsets.size - 1, int(offsets[1])
        cuts = [0, n // 4, n // 4 + n // 3, n]
        builder = msbwt.RleBWT(device=0)
        rles = [builder.build_from_reads((flat, offsets[lo:hi + 1])) for lo, hi in zip(cuts[:-1], cuts[1:])]
        reads = flat.reshape(n, length)
        _parts["reads"] = [reads[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        _parts["rles"] = rles
        _parts["index"] = merged(rles)
        _parts["census"] = {}
    return _parts


def parts_census(k):
    p = three_parts()
    if k not in p["census"]:
        words, m = join([census_of_matrix(r, k) for r in p["reads"]])
        words.setflags(write=False)
        m.setflags(write=False)
        p["census"][k] = (words, m)
    return p["census"][k]


@pytest.mark.parametrize("k", [1, 2, 3, 16, 17, 31, 32])
def test_k_values(k):
    b = three_parts()["index"]
    assert b.get_total_size() > 2 * msbwt.source_block_rows() + 1
    words, m = parts_census(k)
    total = m.sum(axis=1)
    narrow = msbwt.source_narrow_rows()
    assert (total > narrow).all() if k <= 3 else (total <= narrow).any()  # small k: through the checkpoints; large k: from the bytes
    check_spectrum(b, k, words, m, bins=(256,))
    w, c, l = check_dump(b, k, words, m)
    check_against_the_composition(b, k, w, c, l)
    lo, hi = [1, 0, 0], [None, 0, None]  # in part 0, never in part 1
    w, c, l = check_dump(b, k, words, m, lo, hi)
    check_against_the_composition(b, k, w, c, l, lo, hi)
    assert k <= 3 or 0 < len(w) < len(words)


# ---- 3. the border between the two counting paths, in closed form ----

def border_case(tmp_path, t, off, tag):
    """Homopolymer reads of length 3 in three inputs: t reads AAA split 1/2, 1/3 and the rest, one read TTT in each (an input of one
    letter alone would run its '$' block into the letter's own in the RLE), and as many reads CCC in input 1 as put the range of AAA --
    which starts 3 t + n_C + 3 rows into the index: behind the '$' rows and the rows A$.. and AA$.. -- at `off` rows past a multiple
    of the checkpoint block."""
    block = msbwt.source_block_rows()
    split = [t // 2, t // 3, t - t // 2 - t // 3]
    n_c = (off - 3 * t - 3) % block
    inputs = [{"A": split[0], "T": 1}, {"A": split[1], "C": n_c, "T": 1}, {"A": split[2], "T": 1}]
    rles = [homopolymer_rle(counts, 3, str(tmp_path / ("%s_%d.npy" % (tag, i)))) for i, counts in enumerate(inputs)]
    return merged(rles), split, n_c


def border_totals():
    narrow, block = msbwt.source_narrow_rows(), msbwt.source_block_rows()
    return [narrow - 1, narrow, narrow + 1, block - 1, block, block + 1]


@pytest.mark.parametrize("which", range(6))
def test_border_between_the_two_counting_paths(tmp_path, which):
    t = border_totals()[which]
    block = msbwt.source_block_rows()
    for off in (0, 1, 15, 16, 17, block - 1):
        b, split, n_c = border_case(tmp_path, t, off, "t%d_o%d" % (t, off))
        assert b.get_total_size() == 4 * (t + n_c + 3)
        for k in (3, 2, 1):
            a_counts = [n * (3 - k + 1) for n in split]
            words, m = [word_of("A" * k)], [a_counts]
            if n_c:
                words.append(word_of("C" * k))
                m.append([0, n_c * (3 - k + 1), 0])
            words.append(word_of("T" * k))
            m.append([3 - k + 1] * 3)
            words, m = np.array(words, dtype=U64), np.array(m, dtype=U64)
            check_spectrum(b, k, words, m, bins=(2, 256, t + 2))
            w, c, l = check_dump(b, k, words, m)
            # the range of A^k: behind the '$' block (t + n_C + 3 rows) and the k - 1 groups of rotations with fewer leading As
            assert int(l[0]) == (t + n_c + 3) + (k - 1) * t and (k != 3 or int(l[0]) % block == off), (t, off, k, l)
            assert int(c[0].sum()) == t * (3 - k + 1)
            exact = check_dump(b, k, words, m, lo=a_counts, hi=a_counts)  # every source at its exact count
            assert exact[0].tolist() == [0]
            assert check_dump(b, k, words, m, lo=[a_counts[0] + 1, 0, 0])[0].size == 0


# ---- 4. predicates ----

def test_predicates(orc):
    sets = three_sets()
    b = merged([naive_rle(orc, s) for s in sets])
    S = 3
    for k in (3, 8, 21):
        words, m = census_of_sets(sets, k)
        total = m.sum(axis=1)
        for s in range(S):  # private to one source: absent elsewhere
            hi = [0] * S
            hi[s] = None
            w, c, _ = check_dump(b, k, words, m, None, hi)
            assert (k == 3 or len(w) >= 1) and (c[:, s] > 0).all() and not np.delete(c, s, axis=1).any()  # (all three hold nearly every 3-mer)
        w, c, _ = check_dump(b, k, words, m, [1] * S, None)  # present in all
        assert len(w) >= 1 and (c > 0).all()
        check_dump(b, k, words, m, [2, 0, 0], [None, 0, 0])  # at least twice in 0, never elsewhere
        check_dump(b, k, words, m, [0, 1, 0], [3, 2, NO_LIMIT], 2, 5)  # everything at once; NO_LIMIT spelt out
        for lo_t, hi_t in ((2, None), (1, 1), (3, 7)):  # a total window only: the plain dump with that window
            w, c, l = check_dump(b, k, words, m, None, None, lo_t, hi_t)
            pw, pc, pl = b.enumerate_kmers(k, min_count=lo_t, max_count=hi_t, ranges=True)
            assert np.array_equal(w, pw) and np.array_equal(c.sum(axis=1, dtype=U64), pc) and np.array_equal(l, pl)
        assert np.array_equal(b.enumerate_kmers_by_source(k, min_total=0)[0], words)  # 0 is 1
        # the sum of the minima equal to a k-mer's exact total: the walk prunes at that width and must keep it
        shared = np.flatnonzero((m > 0).sum(axis=1) >= 2)
        i = int(shared[np.argmax(total[shared])])
        w, c, _ = check_dump(b, k, words, m, m[i].tolist(), None)
        assert int(words[i]) in w.tolist()
        info = b.spectrum_info()
        assert info["nodes"][k] == int((total >= total[i]).sum()) < len(words)  # pruned at the sum of the minima: what reached the sink
        # impossible: nothing emitted, nothing written
        n = C.c_uint64(77)
        buf = np.full(8, 9, dtype=U64)
        lo, hi = np.array([10 ** 9, 0, 0], dtype=U64), np.array([NO_LIMIT, 0, 0], dtype=U64)
        assert _lib.lib().msbwt_rle_enumerate_kmers_by_source(b._h, k, _ptr(lo), _ptr(hi), 0, 0, 1, _ptr(buf), None, None, 8, C.byref(n)) == 0
        assert n.value == 0 and (buf == 9).all()
        assert check_dump(b, k, words, m, None, [0] * S)[0].size == 0  # absent from every source
    # min > max on a loaded index, and the other argument guards
    lib, n = _lib.lib(), C.c_uint64(77)
    before = b.spectrum_info()["ms"]
    lo, hi = np.array([1, 5, 0], dtype=U64), np.array([NO_LIMIT, 4, 0], dtype=U64)
    hist = np.zeros(3 * 8, dtype=U64)
    assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, 3, _ptr(lo), _ptr(hi), 0, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert b"min_counts[1]" in lib.msbwt_rle_last_error(b._h)
    assert lib.msbwt_rle_enumerate_kmers_by_source_device(b._h, 3, _ptr(lo), _ptr(hi), 0, 0, 1, None, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, 3, None, None, 5, 2, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
    for k in (0, 33, 1000):
        assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, k, None, None, 0, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_kmer_spectrum_by_source(b._h, k, _ptr(hist), 8, None, None, None) == _lib.ERR_INVALID_ARG
    for bins in (0, 1):
        assert lib.msbwt_rle_kmer_spectrum_by_source(b._h, 3, _ptr(hist), bins, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_kmer_spectrum_by_source(b._h, 3, None, 8, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, 3, None, None, 0, 0, 1, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, 3, None, None, 0, 0, 1, None, None, None, 5, C.byref(n)) == _lib.ERR_INVALID_ARG  # a capacity and no buffer
    assert n.value == 77 and not hist.any() and b.spectrum_info()["ms"] == before  # refused before anything ran
    assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, 3, None, None, 5, 0, 1, None, None, None, 0, C.byref(n)) == 0 and n.value < 77  # max_total 0: no limit
    assert lib.msbwt_rle_kmer_spectrum_by_source(b._h, 3, _ptr(hist), 8, None, None, None) == 0 and hist.any()  # the three outputs beside the histogram are optional


# ---- 5. the capacity pattern of both forms ----

def test_capacity_pattern_of_both_forms():
    import torch
    dev = torch.device("cuda:0")
    b = three_parts()["index"]
    k, S = 17, 3
    words, m = parts_census(k)
    lo, hi = [1, 1, 0], [None, None, 2]
    keep = passes(m, lo, hi)
    n = int(keep.sum())
    assert 100 < n < len(words)
    lib, got_n = _lib.lib(), C.c_uint64(0)
    a_lo, a_hi = np.array(lo, dtype=U64), np.array([NO_LIMIT if x is None else x for x in hi], dtype=U64)
    args = (b._h, k, _ptr(a_lo), _ptr(a_hi), 0, 0)
    before = b.device_bytes()
    # host form
    for srt in (1, 0):
        assert lib.msbwt_rle_enumerate_kmers_by_source(*args, srt, None, None, None, 0, C.byref(got_n)) == 0 and got_n.value == n
        w, c, l = np.full(n + 3, 9, dtype=U64), np.full((n + 3) * S, 9, dtype=U64), np.full(n + 3, 9, dtype=U64)
        got_n.value = 0
        assert lib.msbwt_rle_enumerate_kmers_by_source(*args, srt, _ptr(w), _ptr(c), _ptr(l), n - 1, C.byref(got_n)) == _lib.ERR_INVALID_ARG
        assert got_n.value == n and str(n).encode() in lib.msbwt_rle_last_error(b._h)
        assert (w == 9).all() and (c == 9).all() and (l == 9).all()
        for with_counts, with_l in ((True, True), (False, True), (True, False), (False, False)):
            w[:], c[:], l[:] = 9, 9, 9
            capacity = n if with_counts and with_l else n + 3  # exactly n, and more than n
            assert lib.msbwt_rle_enumerate_kmers_by_source(*args, srt, _ptr(w), _ptr(c) if with_counts else None, _ptr(l) if with_l else None, capacity,
                                                           C.byref(got_n)) == 0
            assert got_n.value == n and (w[n:] == 9).all() and (c[n * S:] == 9).all() and (l[n:] == 9).all()
            order = np.arange(n) if srt else np.argsort(w[:n], kind="stable")
            assert np.array_equal(w[:n][order], words[keep])
            assert np.array_equal(c[:n * S].reshape(n, S)[order], m[keep]) if with_counts else (c == 9).all()
            assert (np.diff(l[:n][order].astype(np.int64)) > 0).all() if with_l else (l == 9).all()
    # device form
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert b.enumerate_kmers_by_source_device(k, None, None, None, 0, lo, hi, stream=stream) == n
    ref_l = b.enumerate_kmers_by_source(k, lo, hi, ranges=True)[2]
    for srt in (True, False):
        bufs = [torch.full((n + 3,), -7, dtype=torch.int64, device=dev), torch.full(((n + 3) * S,), -7, dtype=torch.int64, device=dev),
                torch.full((n + 3,), -7, dtype=torch.int64, device=dev)]
        ptrs = [t.data_ptr() for t in bufs]
        with pytest.raises(MsbwtError) as err:
            b.enumerate_kmers_by_source_device(k, *ptrs, n - 1, lo, hi, sorted=srt, stream=stream)
        assert err.value.code == _lib.ERR_INVALID_ARG and err.value.n == n and str(n) in str(err.value)
        assert all(bool((t == -7).all()) for t in bufs)
        assert b.enumerate_kmers_by_source_device(k, *ptrs, n, lo, hi, sorted=srt, stream=stream) == n
        b.device_status(stream)
        w, c, l = (t.cpu().numpy() for t in bufs)
        assert (w[n:] == -7).all() and (c[n * S:] == -7).all() and (l[n:] == -7).all()
        w, c, l = w[:n].astype(U64), c[:n * S].astype(U64).reshape(n, S), l[:n].astype(U64)
        order = np.arange(n) if srt else np.argsort(w, kind="stable")
        assert np.array_equal(w[order], words[keep]) and np.array_equal(c[order], m[keep]) and np.array_equal(l[order], ref_l)
        only = torch.full((n,), -7, dtype=torch.int64, device=dev)  # counts and l are optional
        assert b.enumerate_kmers_by_source_device(k, only.data_ptr(), None, None, n, lo, hi, sorted=srt, stream=stream) == n
        assert np.array_equal(np.sort(only.cpu().numpy().astype(U64)), words[keep])
    b.device_status(stream)
    assert b.device_bytes() == before


def test_the_plan_is_what_a_call_allocates(orc):
    """msbwt_kmers_by_source_plan against msbwt_rle_spectrum_scratch_bytes, the sum of the allocations the last call really made (its
    arena counts them): the walk's two frontiers, the sink's fixed words, the rank scratch of a sorted call that fills buffers, the
    records staged for a host dump, the spectrum's histograms.  On indexes this small the automatic frontier is rows + 1024 nodes
    whatever is free, so the plan does not depend on the moment the free bytes were read; every allocation here is above the 256
    bytes an allocation is rounded up to."""
    import torch
    free = torch.cuda.mem_get_info(0)[0]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    cases = [(merged([naive_rle(orc, s) for s in three_sets()]), 8, lambda k: census_of_sets(three_sets(), k)), (three_parts()["index"], 17, parts_census)]
    for b, k, census in cases:
        S, total = b.source_count(), b.get_total_size()
        plan = lambda records=0, srt=False: msbwt.kmers_by_source_plan(total, free, S, records, srt)
        assert plan() == msbwt.kmers_by_source_plan(total, 10 ** 9, S) and total + 1024 < 2 ** 20  # the frontier is the index's, not the memory's
        words, m = census(k)
        n = len(words)
        for bins in (64, 256):
            b.kmer_spectrum_by_source(k, bins)
            assert b.spectrum_scratch_bytes() == plan() + 8 * S * bins, (k, bins)
        for srt in (True, False):
            assert b.enumerate_kmers_by_source_device(k, None, None, None, 0, sorted=srt, stream=stream) == n  # counting marks nothing
            assert b.spectrum_scratch_bytes() == plan(), (k, srt)
            bufs = [torch.empty(n * x, dtype=torch.int64, device=dev) for x in (1, S, 1)]
            assert b.enumerate_kmers_by_source_device(k, *[t.data_ptr() for t in bufs], n, sorted=srt, stream=stream) == n
            assert b.spectrum_scratch_bytes() == plan(0, srt), (k, srt)  # device form: no records staged
            b.enumerate_kmers_by_source(k, sorted=srt, ranges=True)
            assert b.spectrum_scratch_bytes() == plan(n, srt), (k, srt)  # host form: word, l and S counts per record
            b.enumerate_kmers_by_source(k, sorted=srt)
            assert b.spectrum_scratch_bytes() == plan(n, srt) - 8 * n, (k, srt)  # ... without l
        lo = [1] * S  # the records staged are those that pass, not those that reach the sink
        few = int(passes(m, lo).sum())
        assert 32 < few < n
        b.enumerate_kmers_by_source(k, lo, ranges=True)
        assert b.spectrum_scratch_bytes() == plan(few, True), k
        assert plan(few, True) - plan(0, True) == 8 * (2 + S) * few and plan(0, True) > plan(0, False)
        b.device_status(stream)


# ---- 6. order ----

def test_order():
    b = three_parts()["index"]
    k = 31
    words, m = parts_census(k)
    lo = [0, 1, 0]
    keep = passes(m, lo)
    first = b.enumerate_kmers_by_source(k, lo, ranges=True)
    second = b.enumerate_kmers_by_source(k, lo, ranges=True)
    assert all(np.array_equal(x, y) for x, y in zip(first, second))
    assert np.array_equal(first[0], words[keep]) and (np.diff(first[0].astype(np.int64)) > 0).all() and len(first[0]) > 1000
    loose = b.enumerate_kmers_by_source(k, lo, sorted=False, ranges=True)
    order = np.argsort(loose[0], kind="stable")
    assert all(np.array_equal(x[order], y) for x, y in zip(loose, first))


# ---- 7. independence of the knobs ----

def results(b, k, full=True):
    lo, hi = [1, 0, 0], [None, 0, None]
    everything = [*b.enumerate_kmers_by_source(k, ranges=True)] if full else []
    return [*b.kmer_spectrum_by_source(k), *b.enumerate_kmers_by_source(k, lo, hi, min_total=2, ranges=True), *everything]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def test_knobs_do_not_matter():
    p = three_parts()
    k = 31
    words, m = parts_census(k)
    b = p["index"]
    want = results(b, k)
    assert np.array_equal(want[7], words) and np.array_equal(want[8], m)
    auto = b.spectrum_info()
    assert auto["retries"] == 0 and auto["descents"] == 0 and auto["chunks"] >= 1
    # the frontier at its minimum: thousands of chunks, retries and re-seeding
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)
    try:
        assert same(results(b, k, full=False), want[:7])
        info = b.spectrum_info()
        assert info["chunks"] > 1 and (info["retries"] >= 1 or info["descents"] >= 1), info
        hist = b.kmer_spectrum_by_source(k)[0]
        info = b.spectrum_info()
        assert np.array_equal(hist, want[0]) and info["chunks"] > 1 and info["nodes"][k] == len(words)
    finally:
        b.set_spectrum_frontier(0)
    forms = {"no pair index": dict(pair_index=0), "run blocks": dict(block_format="runs"), "no direct table": dict(table_depth=0)}
    for form, knobs in forms.items():
        other = msbwt.RleBWT(device=0)
        if "block_format" in knobs:
            other.set_block_format(knobs["block_format"])
        other.load_merged_many(p["rles"], keep_sources=True)
        for name in ("pair_index", "table_depth"):
            if name in knobs:
                getattr(other, "set_" + name)(knobs[name])
        assert other.source_count() == 3 and other.get_block_format() == knobs.get("block_format", "planes")
        assert same(results(other, k), want), form
        seeded = other.spectrum_info()["seed_depth"]
        print("%s: seed depth %d" % (form, seeded))
        if form == "no pair index":
            assert not other.get_pair_index() and seeded > 0  # its flat direct table seeds the walk
        if form == "no direct table":
            assert seeded == 0


# ---- 8. beyond 2^32 rows ----

def test_beyond_2_to_32_rows(tmp_path):
    """4.41e9 merged rows from the three homopolymer inputs of test_gpu_sources.py's case of the same name: the k-mers are c^k, input i
    holds n_i,c (length - k + 1) of them, and the range of c^k starts (k - 1) n_c rows into the block of c.  T's block lies beyond row
    2^32, and at k <= 2 every range is far wider than a checkpoint block.  The walks run under a frontier cap (the automatic frontier
    on this index is the full 2^27 nodes, 6.4 GB per call, which test_gpu_spectrum.py's case takes once)."""
    import time
    import torch
    started = time.perf_counter()
    length = 29
    inputs = [{"A": 5 * 10 ** 7, "C": 3 * 10 ** 7, "T": 10 ** 7}, {"A": 2 * 10 ** 7, "G": 2 * 10 ** 7, "T": 10 ** 7}, {"C": 4 * 10 ** 6, "N": 3 * 10 ** 6}]
    totals = [sum(counts.values()) * (length + 1) for counts in inputs]
    total = sum(totals)
    assert total == 441 * 10 ** 7 > 2 ** 32
    need = msbwt.merge_many_plan(totals) + msbwt.source_index_plan(total, len(inputs))
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        pytest.skip("%.1f GB of HBM free, the merge and the source index take %.1f GB" % (free / 1e9, need / 1e9))
    rles = [homopolymer_rle(counts, length, str(tmp_path / ("in%d.npy" % i))) for i, counts in enumerate(inputs)]
    b = msbwt.RleBWT(device=0)
    t0 = time.perf_counter()
    b.load_merged_many(rles, keep_sources=True)
    t1 = time.perf_counter()
    assert b.get_total_size() == total and b.source_count() == 3
    both = {c: sum(counts.get(c, 0) for counts in inputs) for c in "ACGNT"}
    block, at = {}, sum(both.values())
    for c in "ACGNT":
        block[c] = at
        at += both[c] * length
    b.set_spectrum_frontier(4096)
    before = b.device_bytes()
    for k in (1, 2, 28, 29):
        per = length - k + 1
        want = sorted((word_of(c * k), [counts.get(c, 0) * per for counts in inputs], block[c] + (k - 1) * both[c]) for c in "ACGT")
        assert (max(x[2] for x in want) > 2 ** 32) == (k >= 28) and max(x[2] + sum(x[1]) for x in want) > 2 ** 32  # T's range ends beyond row 2^32, from k = 28 on it starts there
        for srt in (True, False):
            w, c, l = b.enumerate_kmers_by_source(k, sorted=srt, ranges=True)
            got = sorted(zip(w.tolist(), c.tolist(), l.tolist())) if not srt else list(zip(w.tolist(), c.tolist(), l.tolist()))
            assert got == want, (k, srt)
        w, c = b.enumerate_kmers_by_source(k, [0, 1, 0], [0, None, 0])  # private to input 1: G^k
        assert w.tolist() == [word_of("G" * k)] and c.tolist() == [[0, 2 * 10 ** 7 * per, 0]]
        w, c = b.enumerate_kmers_by_source(k, [1, 1, 0])  # in inputs 0 and 1: A^k and T^k, the latter beyond row 2^32
        assert w.tolist() == [word_of("A" * k), word_of("T" * k)]
        hist, sharing, distinct, occurrences = b.kmer_spectrum_by_source(k, 4)
        assert hist.tolist() == [[1, 0, 0, 3], [1, 0, 0, 3], [3, 0, 0, 1]] and sharing.tolist() == [0, 1, 3, 0] and distinct.tolist() == [3, 3, 1]
        assert occurrences.tolist() == [sum(x[1][s] for x in want) for s in range(3)]
    assert b.enumerate_kmers_by_source(30)[0].size == 0
    assert b.device_bytes() == before
    print("set-up %.2f s, load %.2f s, the walks %.2f s" % (t0 - started, t1 - t0, time.perf_counter() - t1))


# ---- 9. the lifetime of the attachment ----

def test_lifetime_of_the_attachment(orc):
    sets = three_sets()
    rles = [naive_rle(orc, s) for s in sets]
    k = 5
    words, m = census_of_sets(sets, k)
    b = msbwt.RleBWT(device=0)
    merged_rle, sources = b.merge_many(rles, return_sources=True)
    b.load_vector(merged_rle)
    bare = b.device_bytes()
    calls = (lambda: b.kmer_spectrum_by_source(k), lambda: b.enumerate_kmers_by_source(k), lambda: b.enumerate_kmers_by_source_device(k, None, None, None, 0))
    for call in calls:
        with pytest.raises(MsbwtError) as err:
            call()
        assert err.value.code == _lib.ERR_NOT_LOADED and "no sources attached" in str(err.value)
    b.set_sources(sources, 3)
    attached = b.device_bytes()
    assert attached == bare + msbwt.source_index_plan(len(sources), 3)
    check_spectrum(b, k, words, m)
    assert b.device_bytes() == attached
    check_dump(b, k, words, m, [0, 0, 1], [None, 0, None])
    assert b.device_bytes() == attached
    b.set_sources(sources, 32)  # more sources than occur: the columns beyond stay zero
    wide = np.concatenate([m, np.zeros((len(m), 29), dtype=U64)], axis=1)
    check_spectrum(b, k, words, wide, bins=(256,))
    check_dump(b, k, words, wide, [1] + [0] * 31, [None] * 3 + [0] * 29)
    b.set_sources(None)
    assert b.source_count() == 0 and b.device_bytes() == bare
    for call in calls:
        with pytest.raises(MsbwtError) as err:
            call()
        assert err.value.code == _lib.ERR_NOT_LOADED and "no sources attached" in str(err.value)
    assert np.array_equal(b.enumerate_kmers(k)[0], words)  # the plain calls answer on
    empty = msbwt.RleBWT(device=0)  # an empty index with an attachment of no rows
    empty.load_vector(EMPTY)
    empty.set_sources(np.zeros(0, dtype=np.uint8), 2)
    hist, sharing, distinct, occurrences = empty.kmer_spectrum_by_source(3, 4)
    assert not hist.any() and hist.shape == (2, 4) and not sharing.any() and not distinct.any() and not occurrences.any()
    assert empty.enumerate_kmers_by_source(3)[0].size == 0
