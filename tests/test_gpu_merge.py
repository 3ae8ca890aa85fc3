"""The merge of two BWTs (csrc/merge.hip) against the builders of the tree: the merge of the BWTs of two read sets is the BWT of
their union, so oracle.naive_bwt, synth.build_msbwt_symbols + synth.rle_encode and build_from_reads on the union give the expected
bytes; they never come from the merge itself.  RLE bytes are compared for equality throughout.

Shapes: the smallest at which each mechanism can fail -- merged totals at the tile's borders with whole tiles from one input, runs
at the digit borders 32 and 1024, reads repeated in both inputs (convergence takes twice the read length), and one closed-form
case beyond 2^32 rows."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest

from rle_random import BORDER_STREAMS, canonical_runs, random_stream, raw_byte_stream
from test_gpu_reads_build import READ_SETS, digits, naive_rle, ragged_set, read_set

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
rle_decode, rle_total = msbwt.rle_bwt.rle_decode, msbwt.rle_bwt.rle_total


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def bwt():
    return msbwt.RleBWT(device=0)


def check_interleave(bits, merged, rle0, rle1):
    """The rows with bit 0, in order, are input 0; those with bit 1 input 1."""
    rows = rle_decode(merged)
    assert bits.size == rows.size and int(bits.sum()) == rle_total(rle1)
    assert np.array_equal(rows[bits == 0], rle_decode(rle0))
    assert np.array_equal(rows[bits == 1], rle_decode(rle1))


# ---- the reference's own cases (src/bwt_util.rs, mod tests) ----

@pytest.mark.parametrize("first,second", [(["CCGT"], ["ACG"]), (["ACCA"], ["CAAA"]), (["ACCA"], ["CA"])])
def test_reference_pairs(bwt, orc, first, second):
    a, b = orc.naive_bwt(first), orc.naive_bwt(second)
    want = orc.naive_bwt(first + second)
    assert np.array_equal(bwt.merge(orc.convert_to_vec(a), orc.convert_to_vec(b)), orc.convert_to_vec(want))
    assert msbwt.bwt_util.pairwise_bwt_merge(a, b, device=0) == want
    assert msbwt.bwt_util.pairwise_bwt_merge(b.encode(), a.encode(), device=0) == want.encode()
    codes = msbwt.bwt_util.pairwise_bwt_merge(orc.convert_stoi(a), orc.convert_stoi(b), device=0)
    assert codes.dtype == np.uint8 and np.array_equal(codes, orc.convert_stoi(want))


def test_reference_fold_one_string_at_a_time(bwt, orc):
    strings = ["A", "AA", "AAA", "AAAA", "AAAAA"]
    want = orc.naive_bwt(strings)
    for order in (strings, strings[::-1]):
        text = orc.naive_bwt(order[:1])
        rle = orc.convert_to_vec(text)
        for s in order[1:]:
            text = msbwt.bwt_util.pairwise_bwt_merge(text, orc.naive_bwt([s]), device=0)
            rle = bwt.merge(rle, orc.convert_to_vec(orc.naive_bwt([s])))
        assert text == want
        assert np.array_equal(rle, orc.convert_to_vec(want))


# ---- ragged sets ----

def ragged_pair(seed):
    a = ragged_set(seed)
    rng = np.random.default_rng(5000 + seed)
    b = ragged_set(100 + seed) + [a[0], a[-1], a[int(rng.integers(0, len(a)))][:5]]
    if seed % 3 == 0:
        b += [a[int(i)] for i in rng.integers(0, len(a), size=5)]
    return a, b


@pytest.mark.parametrize("seed", range(30))
def test_ragged_sets(bwt, orc, seed):
    a, b = ragged_pair(seed)
    ra, rb, want = naive_rle(orc, a), naive_rle(orc, b), naive_rle(orc, a + b)
    ab, bits_ab = bwt.merge(ra, rb, return_interleave=True)
    ba, bits_ba = bwt.merge(rb, ra, return_interleave=True)
    assert np.array_equal(ab, want)
    assert np.array_equal(ba, want)
    check_interleave(bits_ab, ab, ra, rb)
    check_interleave(bits_ba, ba, rb, ra)
    c = ragged_set(200 + seed) + a[:2]
    rc, whole = naive_rle(orc, c), naive_rle(orc, a + b + c)
    assert np.array_equal(bwt.merge(ab, rc), whole)
    assert np.array_equal(bwt.merge(ra, bwt.merge(rb, rc)), whole)


# ---- the interleave ----

def test_equal_rotations_keep_the_first_inputs_rows_first(bwt, orc):
    merged, bits = bwt.merge(naive_rle(orc, ["A"] * 3), naive_rle(orc, ["A"] * 2), return_interleave=True)
    assert np.array_equal(merged, naive_rle(orc, ["A"] * 5))
    assert bits.tolist() == [0, 0, 0, 1, 1] + [0, 0, 0, 1, 1]  # the '$' block, then the 'A' block


# ---- tile borders ----

def reads_of(want, seed):
    """Reads whose symbols and terminators number `want`."""
    rng = np.random.default_rng(seed)
    lengths = []
    while sum(lengths) + len(lengths) < want - 60:
        lengths.append(int(rng.integers(0, 58)))
    lengths.append(want - sum(lengths) - len(lengths) - 1)
    assert sum(lengths) + len(lengths) == want
    return [np.array([1, 2, 3, 5, 4], dtype=np.uint8)[rng.choice(5, size=n, p=[0.3, 0.2, 0.2, 0.25, 0.05])] for n in lengths]


_border = {}


def border_case(want):
    """(reads, the CPU builder's RLE bytes of them all), computed once per total."""
    if want not in _border:
        import synth
        reads = reads_of(want, 70 + want)
        expected = synth.rle_encode(synth.build_msbwt_symbols(reads, 2))
        expected.setflags(write=False)
        _border[want] = (reads, expected)
    return _border[want]


@pytest.mark.parametrize("split", ["first", "second", "even"])
@pytest.mark.parametrize("delta", [-1, 0, 1, "two tiles and a row"])
def test_totals_at_the_tile_border(bwt, delta, split):
    tile = msbwt.merge_tile()
    want = 2 * tile + 1 if isinstance(delta, str) else tile + delta
    reads, expected = border_case(want)
    cut = {"first": len(reads) - 1, "second": 1, "even": len(reads) // 2}[split]  # whole tiles come from one input at the first two
    ra, rb = bwt.build_from_reads(reads[:cut]), bwt.build_from_reads(reads[cut:])
    assert rle_total(ra) + rle_total(rb) == want
    merged, bits = bwt.merge(ra, rb, return_interleave=True)
    assert np.array_equal(merged, expected)
    check_interleave(bits, merged, ra, rb)


def test_a_single_empty_read_and_an_empty_input(bwt, orc):
    tile = msbwt.merge_tile()
    reads, _ = border_case(tile)
    big = bwt.build_from_reads(reads)
    import synth
    want = synth.rle_encode(synth.build_msbwt_symbols(reads + [np.empty(0, dtype=np.uint8)], 2))
    dollar = naive_rle(orc, [""])
    assert np.array_equal(bwt.merge(dollar, big), want)
    assert np.array_equal(bwt.merge(big, dollar), want)
    empty = np.empty(0, dtype=np.uint8)
    for a, b in ((empty, big), (big, empty)):
        merged, bits = bwt.merge(a, b, return_interleave=True)
        assert np.array_equal(merged, big)
        assert bits.size == tile and int(bits.sum()) == rle_total(b)
    assert bwt.merge(empty, empty).size == 0
    # an input that is not canonical comes back canonical
    loose = np.array([1 | 2 << 3, 1 | 0 << 3, 0 | 1 << 3, 0 | 0 << 3, 0 | 0 << 3], dtype=np.uint8)  # AA, then '$' with two empty digits
    assert np.array_equal(bwt.merge(loose, empty), orc.convert_to_vec("AA$"))


# ---- the inputs' places in the one symbol array ----

def tiny_reads(total, seed):
    """Reads of at most five letters whose symbols and terminators number `total` (none for 0, one empty read for 1)."""
    rng = np.random.default_rng(seed)
    sizes = [6] * (total // 6) + [total % 6] * (total % 6 > 0)
    return ["".join(rng.choice(list("ACGT"), size=n - 1)) for n in sizes]


@pytest.mark.parametrize("total1", [0, 1, 16])
@pytest.mark.parametrize("total0", [15, 16, 17])
def test_inputs_around_a_16_byte_border(bwt, orc, total0, total1):
    """Both inputs are decoded into one array, each at a 16-byte border: one symbol short of a border, at it and one past it, then
    an input that is empty (its first symbol, which the kernels load, is past the array), a single '$' or a whole line."""
    a, b = tiny_reads(total0, 10 * total0 + total1), tiny_reads(total1, 500 + 10 * total0 + total1)
    ra, rb = naive_rle(orc, a), naive_rle(orc, b) if b else np.empty(0, dtype=np.uint8)
    assert rle_total(ra) == total0 and rle_total(rb) == total1
    want = naive_rle(orc, a + b)
    for first, second in ((ra, rb), (rb, ra)):
        merged, bits = bwt.merge(first, second, return_interleave=True)
        assert np.array_equal(merged, want)
        check_interleave(bits, merged, first, second)
        assert bwt.merge_info()["iterations"] >= 1


# ---- convergence ----

def test_convergence_takes_longer_than_the_read_length(bwt, orc):
    rng = np.random.default_rng(9)
    read = "".join(rng.choice(list("ACGT"), size=60))
    a = [read] * 40 + [read[:59] + c for c in "ACGTN" if c != read[59]][:2] + [read[:59]]
    b = [read] * 40 + [read[:59] + c for c in "ACGTN" if c != read[59]][2:] + [read[:30]]
    merged = bwt.merge(naive_rle(orc, a), naive_rle(orc, b))
    assert bwt.merge_info()["iterations"] > 61  # rotations of the repeated read are told apart only after a whole turn
    assert np.array_equal(merged, naive_rle(orc, a + b))


# ---- runs ----

def test_runs_at_the_digit_borders(bwt, orc):
    for n0, n1 in ((16, 16), (31, 1), (512, 512), (1023, 1), (1, 31)):
        got = bwt.merge(naive_rle(orc, ["A"] * n0), naive_rle(orc, ["A"] * n1))
        assert np.array_equal(got, orc.convert_to_vec("A" * (n0 + n1) + "$" * (n0 + n1))), (n0, n1)
    got = bwt.merge(naive_rle(orc, ["A"] * 16), naive_rle(orc, ["A"] * 16))
    assert digits(got) == [(1, 0), (1, 1), (0, 0), (0, 1)]
    got = bwt.merge(naive_rle(orc, ["A"] * 512), naive_rle(orc, ["A"] * 512))
    assert digits(got) == [(1, 0), (1, 0), (1, 1), (0, 0), (0, 0), (0, 1)]


def test_runs_beyond_1024(bwt):
    import synth
    first, second = ["AAA"] * 600 + ["AAC", "GAAA"], ["AAA"] * 500 + ["T", "", "AAAA"]
    codes = lambda reads: [msbwt.string_util.convert_stoi(r) for r in reads]
    expected = synth.rle_encode(synth.build_msbwt_symbols(codes(first + second), 2))
    got = bwt.merge(bwt.build_from_reads(first, ascii=True), bwt.build_from_reads(second, ascii=True))
    assert np.array_equal(got, expected)
    d = digits(got)
    assert any(d[i][0] == d[i + 1][0] == d[i + 2][0] for i in range(len(d) - 2))


def test_two_runs_join_into_one_and_split_runs_decode_the_same(bwt, orc):
    ra, rb = naive_rle(orc, ["A"] * 600), naive_rle(orc, ["A"] * 500)
    want = orc.convert_to_vec("A" * 1100 + "$" * 1100)
    got = bwt.merge(ra, rb)
    assert np.array_equal(got, want)
    assert [s for s, _ in digits(got)] == [1, 1, 1, 0, 0, 0]  # one run of 1100: three digits of one symbol in a row
    # the same rows from ONE input that is not canonical: the 'A's as 600 and 500 with an empty '$' run between the two byte groups,
    # the '$'s as 76 + 32 * 32 with two empty digits on top
    assert digits(ra)[:2] == [(1, 24), (1, 18)] and digits(rb)[:2] == [(1, 20), (1, 15)]
    loose = np.array([1 | 24 << 3, 1 | 18 << 3, 0, 1 | 20 << 3, 1 | 15 << 3, 0 | 12 << 3, 0 | 2 << 3, 0 | 1 << 3, 0, 0], dtype=np.uint8)
    ref = orc.OracleRleBWT()
    ref.load_vector(loose)
    assert ref.get_symbol_count(1) == 1100 and ref.get_symbol_count(0) == 1100 == rle_total(loose) // 2
    empty = np.empty(0, dtype=np.uint8)
    assert np.array_equal(bwt.merge(loose, empty), want)
    assert np.array_equal(bwt.merge(empty, loose), want)


# ---- the decoder on streams that are no BWT of anything ----

DECODER_STREAMS = dict(BORDER_STREAMS, mixed=lambda: random_stream(31, 20000, "mixed"),
                       **{"raw %d" % s: (lambda s=s: raw_byte_stream(s, 5000)) for s in range(4)})


@pytest.mark.parametrize("name", sorted(DECODER_STREAMS))
def test_any_stream_merged_with_nothing_comes_back_canonical(bwt, orc, name):
    """A merge with an empty input needs no read set behind the other one: it decodes the stream and encodes the symbols again.
    Zero digits, runs of no symbols, a run's digits across a thread's (16 bytes) and a tile's (4096) border of the decoder, and
    sub-runs on both sides of 1024 symbols, where a second kernel takes over."""
    import synth
    stream, empty = DECODER_STREAMS[name](), np.empty(0, dtype=np.uint8)
    want = synth.rle_encode(orc.decompress(stream))
    assert np.array_equal(canonical_runs(stream), want)  # (the restatement that stands in where a stream is too long to decode)
    assert np.array_equal(bwt.merge(stream, empty), want)
    assert np.array_equal(bwt.merge(empty, stream), want)
    assert np.array_equal(bwt.merge_many([stream]), want)


# ---- read sets ----

@pytest.mark.parametrize("name", sorted(READ_SETS))
def test_read_sets_cut_in_half(orc, name):
    (flat, offsets), expected = read_set(name)
    n = offsets.size - 1
    b = msbwt.RleBWT(device=0)
    ra = b.build_from_reads((flat, offsets[:n // 2 + 1]))
    rb = b.build_from_reads((flat, offsets[n // 2:]))
    assert np.array_equal(b.merge(ra, rb), expected)
    b.load_merged(ra, rb)
    ref = orc.OracleRleBWT()
    ref.load_vector(expected)
    rng = np.random.default_rng(3)
    length = int(offsets[1])
    reads = flat.reshape(n, length)
    rows, starts = rng.integers(0, n, size=2000), rng.integers(0, length - 30, size=2000)
    derived = np.stack([reads[r, s:s + 31] for r, s in zip(rows, starts)])
    random31 = np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=(2000, 31))]
    kmers = np.ascontiguousarray(np.concatenate([derived, random31]))
    want = ref.count_kmers(kmers)
    assert int((want > 0).sum()) >= 2000
    assert b.get_total_size() == ref.get_total_size()
    assert np.array_equal(b.count_kmers(kmers), want)


# ---- beyond 2^32 rows ----

LETTERS = {"A": 1, "C": 2, "G": 3, "N": 4, "T": 5}


def homopolymer_runs(counts, length):
    """The BWT of counts[c] reads c^length per letter c, as (symbol, count) runs: the '$' block holds every read's last symbol,
    reads in order; a letter's block is c^(n (length - 1)) $^n."""
    runs = [(LETTERS[c], counts.get(c, 0)) for c in "ACGNT"]
    for c in "ACGNT":
        runs += [(LETTERS[c], counts.get(c, 0) * (length - 1)), (0, counts.get(c, 0))]
    return [r for r in runs if r[1]]


def homopolymer_bit(row, first, second, length):
    """Whether merged row `row` is the second input's: per block of equal rotations the first input's rows come first."""
    at = 0
    for c in "ACGNT":  # the '$' block
        n0, n1 = first.get(c, 0), second.get(c, 0)
        if row < at + n0 + n1:
            return int(row - at >= n0)
        at += n0 + n1
    for c in "ACGNT":  # a letter's block: `length` groups of n0 + n1 equal rotations
        n0, n1 = first.get(c, 0), second.get(c, 0)
        if row < at + (n0 + n1) * length:
            return int((row - at) % (n0 + n1) >= n0)
        at += (n0 + n1) * length
    raise IndexError(row)


def test_homopolymer_closed_form_at_a_small_size(bwt, orc):
    first, second, length = {"A": 3, "C": 2, "T": 1}, {"A": 1, "G": 2, "T": 2}, 4
    reads = lambda counts: [c * length for c in "ACGNT" for _ in range(counts.get(c, 0))]
    text = lambda runs: "".join("$ACGNT"[s] * n for s, n in runs)
    both = {c: first.get(c, 0) + second.get(c, 0) for c in "ACGNT"}
    assert text(homopolymer_runs(first, length)) == orc.naive_bwt(reads(first))
    assert text(homopolymer_runs(both, length)) == orc.naive_bwt(reads(first) + reads(second))
    merged, bits = bwt.merge(naive_rle(orc, reads(first)), naive_rle(orc, reads(second)), return_interleave=True)
    assert np.array_equal(merged, orc.convert_to_vec(text(homopolymer_runs(both, length))))
    assert bits.tolist() == [homopolymer_bit(i, first, second, length) for i in range(bits.size)]


def test_beyond_2_to_32_rows(tmp_path):
    """5.1e9 merged rows from inputs of a few dozen RLE bytes; read length 29, 30 iterations.  Measured on an MI355X: the merge
    call takes 0.6 s (iterate 0.51 s, the 640 MB of interleave bits to the host 0.04 s) and the checks after it 0.8 s, so the read
    length stays at 29; where this test is the first of its process to start torch, that start-up adds about 13 s before the call."""
    started = time.perf_counter()
    import torch
    first, second, length = {"A": 6 * 10 ** 7, "C": 3 * 10 ** 7, "T": 10 ** 7}, {"A": 2 * 10 ** 7, "G": 3 * 10 ** 7, "T": 2 * 10 ** 7}, 29
    both = {c: first.get(c, 0) + second.get(c, 0) for c in "ACGNT"}
    total0, total1 = sum(first.values()) * (length + 1), sum(second.values()) * (length + 1)
    total = total0 + total1
    assert total == 51 * 10 ** 8 > 2 ** 32
    need = msbwt.merge_plan(total0, total1)
    free, _ = torch.cuda.mem_get_info(0)
    if free < need + need // 4:
        pytest.skip("%.1f GB of HBM free, the merge takes %.1f GB" % (free / 1e9, need / 1e9))
    rle = {}
    for name, counts in (("first", first), ("second", second), ("both", both)):
        path = str(tmp_path / (name + ".npy"))
        msbwt.bwt_converter.save_bwt_runs_numpy(homopolymer_runs(counts, length), path)
        rle[name] = np.array(np.load(path))
        assert rle_total(rle[name]) == sum(counts.values()) * (length + 1)
    b = msbwt.RleBWT(device=0)
    out = np.zeros(rle["first"].size + rle["second"].size, dtype=np.uint8)
    bits = np.zeros((total + 7) // 8, dtype=np.uint8)
    got = C.c_uint64(0)
    t0 = time.perf_counter()
    rc = _lib.lib().msbwt_rle_merge(b._h, rle["first"].ctypes.data_as(C.c_void_p), rle["first"].size, rle["second"].ctypes.data_as(C.c_void_p), rle["second"].size,
                                    out.ctypes.data_as(C.c_void_p), out.size, C.byref(got), bits.ctypes.data_as(C.c_void_p))
    print("merge of %d rows: %.2f s after %.2f s of set-up, %s" % (total, time.perf_counter() - t0, t0 - started, b.merge_info()))
    assert rc == 0, _lib.lib().msbwt_rle_last_error(b._h)
    assert np.array_equal(out[:got.value], rle["both"])
    assert int(np.bitwise_count(bits).sum(dtype=np.uint64)) == total1 == 7 * 10 ** 7 * 30
    borders = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, total - 1, 0]
    at = 0
    for c in "ACGNT":  # the borders between the inputs' rows in the groups around row 2^32, and those of every '$' group
        n0, n1 = first.get(c, 0), second.get(c, 0)
        borders += [at + n0 - 1, at + n0, at + n0 + n1 - 1]
        at += n0 + n1
    assert at == sum(both.values())
    for c in "ACGNT":
        n0, n1 = first.get(c, 0), second.get(c, 0)
        for group in range(length if n0 + n1 else 0):
            lo = at + group * (n0 + n1)
            if lo + n0 + n1 > 2 ** 32 - 2 * 10 ** 8:
                borders += [lo, lo + n0 - 1, lo + n0, lo + n0 + n1 - 1]
        at += (n0 + n1) * length
    assert at == total
    borders = sorted(set(r for r in borders if 0 <= r < total))
    assert any(r > 2 ** 32 for r in borders)
    for row in borders:
        assert (int(bits[row >> 3]) >> (row & 7)) & 1 == homopolymer_bit(row, first, second, length), row
    assert b.merge_info()["iterations"] >= length
    print("checks done %.2f s after the start" % (time.perf_counter() - started))


# ---- errors ----

def _raw_merge(handle, a, b, out, cap):
    length = C.c_uint64(0)
    rc = _lib.lib().msbwt_rle_merge(handle, a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, out.ctypes.data_as(C.c_void_p), cap,
                                    C.byref(length), None)
    return rc, length.value


def test_errors_leave_the_handle_usable(bwt, orc):
    a, b = ragged_pair(21)
    ra, rb, expected = naive_rle(orc, a), naive_rle(orc, b), naive_rle(orc, a + b)
    for bad in (np.array([1 | 1 << 3, 6 | 1 << 3], dtype=np.uint8), np.array([7 | 3 << 3], dtype=np.uint8)):
        for pair in ((bad, rb), (ra, bad)):
            with pytest.raises(msbwt.MsbwtError) as err:
                bwt.merge(*pair)
            assert err.value.code == _lib.ERR_INVALID_SYMBOL
    out = np.full(expected.size + 8, 0xAB, dtype=np.uint8)
    rc, need = _raw_merge(bwt._h, ra, rb, out, expected.size - 1)
    assert rc == _lib.ERR_INVALID_ARG and need == expected.size
    assert (out == 0xAB).all()
    rc, need = _raw_merge(bwt._h, ra, rb, out, expected.size)
    assert rc == 0 and need == expected.size and np.array_equal(out[:need], expected) and (out[need:] == 0xAB).all()
