"""Exact expectations for indexes beyond 2^32 rows, from sets of about 10^6 rows: the helpers of tests/test_gpu_scaled_copies.py and
the CPU proof that what they expect is right.  Nothing here needs a GPU.

Let S be a read set and S x c the set that holds every read of S c times.  Equal reads are adjacent in the sorted text, equal
suffixes are ordered by text position and equal rotations from different inputs keep input order, so, row for row:

* BWT(S x c) is BWT(S) with every row repeated c times;
* the source vector of the merge of S0 x c, S1 x c, ... is that of the merge of S0, S1, ... with every entry repeated c times;
* the range [l, h) of a k-mer becomes [c l, c h).

The tests below check all three at c = 1, 2, 5 and 33 against oracle.naive_bwt, synth.rle_encode, the restated merge iteration of
test_gpu_merge_many.expected_sources and the CPU oracle, with the copies shuffled through the input, on ragged sets of a few
thousand rows with N, duplicates, prefixes, empty reads and reads shared between the inputs."""
import importlib

import numpy as np
import pytest

from test_gpu_merge_many import expected_sources
from test_gpu_sparse import oracle_ranges
from test_gpu_spectrum import census_of_texts

msbwt = importlib.import_module("rust-msbwt_amd")
rle_total = msbwt.rle_bwt.rle_total
unpack_2bit = msbwt.rle_bwt.unpack_2bit
EMPTY = np.empty(0, dtype=np.uint8)
U64 = np.uint64
LONGEST = 41  # two key words of 21 symbols: the builder sorts in 16 radix passes
CODES = np.array([1, 2, 3, 5, 4], dtype=np.uint8)  # A C G T N
CODE_P = [0.3, 0.2, 0.2, 0.25, 0.05]
COPIES = (1, 2, 5, 33)
# the row counts of the small sets of tests/test_gpu_scaled_copies.py: times 4369 and 4096 they are 2^32 - 1, 2^32 and 4 505 600 000
# rows (the builder), 600 000 + 500 000 (the merge of two) and 500 000 + 400 000 + 200 000 (the merge of three)
GPU_ROWS = (983055, 1048576, 1100000, 600000, 500000, 400000, 200000)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---- the helpers ----

def random_reads(rng, lengths):
    """One read of symbol codes per entry of `lengths`."""
    lengths = np.asarray(lengths, dtype=np.int64)
    flat = CODES[rng.choice(5, size=int(lengths.sum()), p=CODE_P)]
    return np.split(flat, np.cumsum(lengths)[:-1]) if lengths.size else []


def copy_set(rows, seed, shared=()):
    """A read set (list of arrays of symbol codes) whose symbols and terminators number `rows` exactly: reads of 0..41 symbols over
    ACGTN, about 2 % of them exact duplicates and 2 % prefixes of others (the first one the empty prefix), then the reads of
    `shared`, then short and empty reads up to the total."""
    rng = np.random.default_rng(seed)
    shared = [np.asarray(r, dtype=np.uint8) for r in shared]
    budget = rows - sum(r.size + 1 for r in shared)
    assert budget >= 2 * (LONGEST + 1), "too few rows for the shared reads and a tail"
    lengths = rng.integers(0, LONGEST + 1, size=budget // 12 + 1)
    room = budget - budget // 16 - 2 * (LONGEST + 1)  # the sixteenth: duplicates and prefixes (about 4 % of the rows) and the tail
    taken = int(np.searchsorted(np.cumsum(lengths + 1), room, side="right"))
    base = random_reads(rng, lengths[:taken])
    reads = list(base)
    extras = max(1, len(base) // 50)
    if base:
        reads += [base[int(i)] for i in rng.integers(0, len(base), size=extras)]
        for j, i in enumerate(rng.integers(0, len(base), size=extras)):
            r = base[int(i)]
            reads.append(r[:int(rng.integers(0, r.size + 1)) if j else 0])
    reads += shared
    left = rows - sum(r.size + 1 for r in reads)
    assert left >= 2, "the duplicates and prefixes took more than their share"
    more = lengths[taken:]
    more = more[:int(np.searchsorted(np.cumsum(more + 1), left - 2 * (LONGEST + 1), side="right"))]  # (none if that is negative)
    reads += random_reads(rng, more)
    left -= int(more.sum()) + more.size
    reads.append(EMPTY)
    left -= 1
    while left > 8:
        reads += random_reads(rng, [int(rng.integers(0, 6))])
        left -= reads[-1].size + 1
    reads += random_reads(rng, [left - 1])
    assert sum(r.size + 1 for r in reads) == rows
    return reads


def runs_of(symbols):
    """(symbols, lengths) of the runs of an array of symbols."""
    s = np.ascontiguousarray(symbols, dtype=np.uint8)
    if s.size == 0:
        return s, np.zeros(0, dtype=U64)
    heads = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return s[heads], np.diff(np.append(heads, s.size)).astype(U64)


def scaled_rle(symbols, c, path):
    """The RLE bytes of `symbols` with every symbol repeated c times: the runs of `symbols`, their lengths times c, through the host
    codec (bwt_converter.save_bwt_runs_numpy) and read back."""
    syms, lengths = runs_of(symbols)
    msbwt.bwt_converter.save_bwt_runs_numpy(zip(syms.tolist(), (lengths * U64(c)).tolist()), path)
    return np.array(np.load(path))


def tiled(reads, c):
    """(flat, offsets) of the whole set c times in a row: the copies of one read lie a whole set apart."""
    one = np.concatenate(list(reads) + [EMPTY])
    starts = np.zeros(len(reads) + 1, dtype=U64)
    np.cumsum([r.size for r in reads], out=starts[1:])
    offsets = np.empty(len(reads) * c + 1, dtype=U64)
    np.add((np.arange(c, dtype=U64) * U64(one.size))[:, None], starts[None, :-1], out=offsets[:-1].reshape(c, len(reads)))
    offsets[-1] = c * one.size
    return np.tile(one, c), offsets


def census_of_codes(reads, k):
    """(sorted words, their counts) of the ACGT-only windows of length k <= 32 of reads given as arrays of symbol codes, by numpy:
    test_gpu_spectrum.census_of_texts for ragged sets of 10^6 symbols."""
    two_bit = np.full(6, 4, dtype=np.uint8)
    two_bit[[1, 2, 3, 5]] = [0, 1, 2, 3]
    text = np.concatenate([np.append(r, 0).astype(np.uint8) for r in reads] + [EMPTY])  # every read, then its '$'
    if text.size < k:
        return np.zeros(0, dtype=U64), np.zeros(0, dtype=U64)
    sym = two_bit[text]
    bad = np.concatenate([[0], np.cumsum(sym == 4)])
    ok = bad[k:] == bad[:-k]  # window [i, i + k) holds no '$' and no N
    words = np.zeros(text.size - k + 1, dtype=U64)
    for j in range(k):
        words = (words << U64(2)) | (sym[j:j + words.size] & 3).astype(U64)
    words, counts = np.unique(words[ok], return_counts=True)
    return words, counts.astype(U64)


def counts_in(words, own_words, own_counts):
    """The counts of `words` in a census (own_words, own_counts); 0 where it does not hold them."""
    if own_words.size == 0:
        return np.zeros(words.size, dtype=U64)
    at = np.minimum(np.searchsorted(own_words, words), own_words.size - 1)
    return np.where(own_words[at] == words, own_counts[at], U64(0)).astype(U64)


def first_row_that_is_not_repeated(big, small, c):
    """-1 if big == np.repeat(small, c): big reshaped to (-1, c) has constant rows and its column 0 is `small`.  Compared eight
    bytes at a time: a row is constant exactly if each of its c / 8 words is its first byte in all eight places."""
    assert big.dtype == small.dtype == np.uint8 and big.size == small.size * c and c % 8 == 0
    words = big.view(U64).reshape(small.size, c // 8)
    want = small.astype(U64) * U64(0x0101010101010101)
    for lo in range(0, small.size, 1 << 15):
        bad = np.flatnonzero((words[lo:lo + (1 << 15)] != want[lo:lo + (1 << 15), None]).any(axis=1))
        if bad.size:
            return lo + int(bad[0])
    return -1


def as_text(read):
    return "".join("$ACGNT"[int(s)] for s in read)


def bwt_symbols(reads):
    import synth
    return synth.build_msbwt_symbols(list(reads), 2)


# ---- the proof ----

def small_inputs(n):
    """n read sets of 1000-1600 rows; reads shared between every pair and among all, one input with extra empty reads."""
    rng = np.random.default_rng(50 + n)
    among_all = [np.where(r == 4, 1, r).astype(np.uint8) for r in random_reads(rng, [30, 41, 7])]  # (no N: their 31-mers count)
    pair = {(i, j): random_reads(rng, [25, 3]) for i in range(n) for j in range(i + 1, n)}
    sets = []
    for i in range(n):
        shared = among_all + [r for key, rs in pair.items() if i in key for r in rs] + ([EMPTY, EMPTY] if i == 1 else [])
        sets.append(copy_set(1000 + 300 * i, 60 + 10 * n + i, shared))
    return sets


def shuffled_copies(reads, c, seed):
    order = np.random.default_rng(seed).permutation(len(reads) * c)
    return [reads[int(i) % len(reads)] for i in order]


@pytest.mark.parametrize("rows", GPU_ROWS + (200, 4097))
def test_copy_set_hits_its_rows_exactly(rows):
    reads = copy_set(rows, 7, shared=random_reads(np.random.default_rng(1), [41, 0, 12]))
    sizes = np.array([r.size for r in reads])
    assert int(sizes.sum()) + len(reads) == rows
    assert sizes.max() <= LONGEST and sizes.min() == 0 and all(r.dtype == np.uint8 for r in reads)
    if rows >= 4097:
        assert sizes.max() == LONGEST
        texts = [r.tobytes() for r in reads]
        assert len(set(texts)) < len(texts) - len(texts) // 100  # duplicates (short reads collide too)
        symbols = np.concatenate(reads)
        share = np.bincount(symbols, minlength=6)[[1, 2, 3, 5, 4]] / symbols.size
        assert np.abs(share - CODE_P).max() < 0.03
    again = copy_set(rows, 7, shared=random_reads(np.random.default_rng(1), [41, 0, 12]))
    assert len(again) == len(reads) and all(np.array_equal(a, b) for a, b in zip(again, reads))


@pytest.mark.parametrize("c", COPIES)
def test_tiled_is_the_set_c_times(c):
    reads = copy_set(300, 3)
    flat, offsets = tiled(reads, c)
    assert offsets.dtype == U64 and offsets.size == len(reads) * c + 1 and flat.size == int(offsets[-1])
    for i in (0, 1, len(reads) - 1, len(reads), len(reads) * c - 1):
        if i < len(reads) * c:
            assert np.array_equal(flat[int(offsets[i]):int(offsets[i + 1])], reads[i % len(reads)]), i
    assert np.all(offsets[1:] >= offsets[:-1])
    flat, offsets = tiled([EMPTY, EMPTY], c)
    assert flat.size == 0 and not offsets.any() and offsets.size == 2 * c + 1


@pytest.mark.parametrize("c", COPIES)
def test_the_bwt_of_the_copies_is_every_row_c_times(orc, tmp_path, c):
    import synth
    for seed in (1, 2):
        reads = copy_set(1500 + 700 * seed, seed)
        symbols = bwt_symbols(reads)
        got = scaled_rle(symbols, c, str(tmp_path / "scaled.npy"))
        assert rle_total(got) == c * symbols.size
        assert np.array_equal(got, synth.rle_encode(np.repeat(symbols, c)))
        copies = shuffled_copies(reads, c, 10 * seed + c)
        assert np.array_equal(got, orc.convert_to_vec(orc.naive_bwt([as_text(r) for r in copies])))
        assert np.array_equal(got, synth.rle_encode(synth.build_msbwt_symbols(copies, 2)))


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("c", COPIES)
def test_the_sources_of_the_copies_are_every_entry_c_times(tmp_path, c, n):
    import synth
    sets = small_inputs(n)
    symbols = [bwt_symbols(s) for s in sets]
    small = expected_sources([synth.rle_encode(s) for s in symbols])
    assert [int(np.count_nonzero(small == i)) for i in range(n)] == [s.size for s in symbols]
    assert np.count_nonzero(small[1:] != small[:-1]) > 100  # (the inputs' rows are mixed)
    # the scaled inputs once as the test on the GPU makes them, once as the BWTs of shuffled copies
    scaled = [scaled_rle(s, c, str(tmp_path / ("in%d.npy" % i))) for i, s in enumerate(symbols)]
    built = [synth.rle_encode(synth.build_msbwt_symbols(shuffled_copies(s, c, 100 * c + i), 2)) for i, s in enumerate(sets)]
    assert all(np.array_equal(a, b) for a, b in zip(scaled, built))
    assert np.array_equal(expected_sources(scaled), np.repeat(small, c))


@pytest.mark.parametrize("c", COPIES)
def test_ranges_and_counts_of_the_copies_are_c_times_those_of_the_set(orc, tmp_path, c):
    reads = sum(small_inputs(3), [])
    symbols = bwt_symbols(reads)
    import synth
    ref, big = orc.OracleRleBWT(), orc.OracleRleBWT()
    ref.load_vector(synth.rle_encode(symbols))
    big.load_vector(scaled_rle(symbols, c, str(tmp_path / "scaled.npy")))
    assert big.get_total_size() == c * ref.get_total_size()
    assert [big.get_symbol_count(s) for s in range(6)] == [c * ref.get_symbol_count(s) for s in range(6)]
    rng = np.random.default_rng(c)
    for k in (1, 3, 12, 31):
        words, counts = census_of_codes(reads, k)
        assert len(words) > (3 if k == 1 else 30) and counts.max() > 1
        pick = rng.choice(len(words), size=min(300, len(words)), replace=False)
        kmers = unpack_2bit(words[pick], k)
        l, h = oracle_ranges(ref, kmers)
        assert np.array_equal(h - l, counts[pick])  # the census of windows is the oracle's count
        bl, bh = oracle_ranges(big, kmers)
        assert np.array_equal(bl, l * U64(c)) and np.array_equal(bh, h * U64(c))
        for q in range(0, len(pick), 37):  # and one symbol at a time through the scalar entry
            lo, hi = 0, big.get_total_size()
            for s in kmers[q][::-1]:
                lo, hi = big.constrain_range(int(s), lo, hi)
            assert (lo, hi) == (c * int(l[q]), c * int(h[q]))
        assert np.array_equal(big.count_kmers(kmers), counts[pick] * U64(c))
        absent = CODES[:4][rng.integers(0, 4, size=(50, k))]
        assert np.array_equal(big.count_kmers(absent), ref.count_kmers(absent) * U64(c))


@pytest.mark.parametrize("k", [1, 2, 12, 31, 32])
def test_census_of_codes_is_the_counter_over_texts(k):
    sets = small_inputs(3)
    reads = sum(sets, [])
    want_words, want_counts = census_of_texts([as_text(r) for r in reads], k)
    words, counts = census_of_codes(reads, k)
    assert np.array_equal(words, want_words) and np.array_equal(counts, want_counts) and len(words) > 0
    total = np.zeros(len(words), dtype=U64)
    for s in sets:  # column by column
        own = dict(zip(*(x.tolist() for x in census_of_texts([as_text(r) for r in s], k))))
        got = counts_in(words, *census_of_codes(s, k))
        assert got.tolist() == [own.get(w, 0) for w in words.tolist()]
        total += got
    assert np.array_equal(total, counts)
    assert counts_in(words, np.zeros(0, dtype=U64), np.zeros(0, dtype=U64)).tolist() == [0] * len(words)


def test_the_word_compare_sees_one_wrong_byte():
    small = np.array([0, 2, 1, 1, 0], dtype=np.uint8)
    big = np.repeat(small, 16)
    assert first_row_that_is_not_repeated(big, small, 16) == -1
    for at, row in ((0, 0), (31, 1), (32, 2), (79, 4)):
        wrong = big.copy()
        wrong[at] ^= 1
        assert first_row_that_is_not_repeated(wrong, small, 16) == row
