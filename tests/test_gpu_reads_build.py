"""The builder from reads (csrc/reads_build.hip) against the two CPU builders of the tree: oracle.naive_bwt (the reference's
naive_bwt restated) and synth.build_msbwt_symbols + synth.rle_encode.  RLE bytes are compared for equality throughout.

Shapes: the smallest at which each mechanism can fail -- read lengths at the key-word borders (21, 42, 63 symbols), suffix counts
at the sort tile's border, piece limits below a bin / between bins / above the total, runs at the digit borders 32 and 1024."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, expand_case

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
ALPHABET = "ACGTN"


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def bwt():
    return msbwt.RleBWT(device=0)


def naive_rle(orc, reads):
    return orc.convert_to_vec(orc.naive_bwt(reads))


def ragged_set(seed):
    """1-40 reads of lengths 0-70 over ACGTN, then duplicates and prefixes of some of them."""
    rng = np.random.default_rng(1000 + seed)
    reads = ["".join(rng.choice(list(ALPHABET), size=int(rng.integers(0, 71)), p=[0.3, 0.2, 0.2, 0.25, 0.05])) for _ in range(int(rng.integers(1, 41)))]
    for _ in range(int(rng.integers(1, 6))):
        r = reads[int(rng.integers(0, len(reads)))]
        reads.append(r)                                        # a duplicate
        reads.append(r[:int(rng.integers(0, len(r) + 1))])     # a prefix (possibly empty, possibly the whole read)
    return reads


# ---- golden ----

def test_two_string_fasta_gives_the_golden_file(tmp_path):
    built = msbwt.create_from_fastx(os.path.join(GOLDEN_DIR, "two_string.fa"), device=0)
    out = str(tmp_path / "two_string.npy")
    msbwt.bwt_converter.save_bwt_numpy(built.rle, out)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN_DIR, "two_string.npy"), "rb").read()
    assert built.get_total_size() == 10 and built.count_kmer(msbwt.string_util.convert_stoi("ACGT")) == 1


def test_reference_naive_bwt_vectors(bwt, orc, golden):
    for case in golden["G3_naive_bwt"]["cases"]:
        got = bwt.build_from_reads(case["strings"], ascii=True)
        assert np.array_equal(got, orc.convert_to_vec(case["bwt"])), case["strings"]


# ---- ragged sets against naive_bwt ----

@pytest.mark.parametrize("seed", range(30))
def test_ragged_sets(bwt, orc, seed):
    reads = ragged_set(seed)
    assert np.array_equal(bwt.build_from_reads(reads, ascii=True), naive_rle(orc, reads))


@pytest.mark.parametrize("length", [20, 21, 22, 41, 42, 43, 62, 63, 64])
def test_read_lengths_at_the_key_word_borders(bwt, orc, length):
    # few distinct reads that agree on long prefixes: ties in word 0 (and 1) are decided in the next word; plus reads one symbol
    # shorter and longer that are prefixes / extensions of them
    rng = np.random.default_rng(length)
    stem = "".join(rng.choice(list("ACGT"), size=length + 1))
    reads = []
    for i in range(24):
        r = list(stem[:length])
        for at in rng.integers(max(0, length - 23), length, size=int(rng.integers(0, 3))):
            r[at] = ALPHABET[int(rng.integers(0, 5))]
        reads.append("".join(r))
    reads += [stem[:length], stem[:length], stem[:length - 1], stem[:length + 1], stem[:21], stem[:20], ""]
    assert all(len(r) == length for r in reads[:26])
    assert np.array_equal(bwt.build_from_reads(reads, ascii=True), naive_rle(orc, reads))


def test_one_long_read_among_short_ones(bwt, orc):
    rng = np.random.default_rng(7)
    long_read = "".join(rng.choice(list(ALPHABET), size=1000))
    reads = ["ACGT", long_read[400:430], long_read, "", long_read[:64], "T"]
    assert np.array_equal(bwt.build_from_reads(reads, ascii=True), naive_rle(orc, reads))


def test_a_single_read_of_length_one(bwt, orc):
    assert np.array_equal(bwt.build_from_reads(["G"], ascii=True), naive_rle(orc, ["G"]))


def test_only_empty_reads(bwt, orc):
    for n in (1, 5, 40):
        assert np.array_equal(bwt.build_from_reads([""] * n, ascii=True), naive_rle(orc, [""] * n))
    assert bwt.build_from_reads([], ascii=True).size == 0


# ---- read sets against the synth builder; piece limits ----

READ_SETS = {"plain_100": (False, 4000, 100), "plain_150": (False, 2700, 150), "repeat_100": (True, 4000, 100), "repeat_150": (True, 2700, 150)}
_cache = {}


def read_set(name):
    """(reads, the CPU builder's RLE bytes), computed once per name."""
    if name not in _cache:
        import synth
        repeats, n, length = READ_SETS[name]
        g = synth.repeat_genome(20000, 5) if repeats else synth.genome(20000, 5)
        reads = synth.reads(g, n, length, 6, 0.005)
        expected = synth.rle_encode(synth.build_msbwt_symbols(reads, 4))
        reads.setflags(write=False)
        expected.setflags(write=False)
        _cache[name] = ((reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)), expected)
    return _cache[name]


@pytest.mark.parametrize("limit", [0, 1000, 65537, 1 << 20])  # automatic; below most bins; a few bins; above the total (~4.1e5)
@pytest.mark.parametrize("name", sorted(READ_SETS))
def test_read_sets_at_every_piece_limit(name, limit):
    reads, expected = read_set(name)
    b = msbwt.RleBWT(device=0)
    b.set_build_piece(limit)
    got = b.build_from_reads(reads)
    assert np.array_equal(got, expected)
    pieces = b.build_stage_ms()["pieces"]
    assert pieces > 100 if limit == 1000 else pieces > 1 if limit == 65537 else pieces == 1


def test_ragged_set_under_a_small_piece_limit(orc):
    reads = ragged_set(3) + ragged_set(4)
    b = msbwt.RleBWT(device=0)
    for limit in (1, 7, 100):
        b.set_build_piece(limit)
        assert np.array_equal(b.build_from_reads(reads, ascii=True), naive_rle(orc, reads)), limit


def test_wide_positions_give_the_same_bytes(monkeypatch):
    reads, expected = read_set("plain_100")
    monkeypatch.setenv("MSBWT_BUILD_WIDE", "1")  # the 64-bit position path of texts beyond 2^32 symbols
    b = msbwt.RleBWT(device=0)
    assert np.array_equal(b.build_from_reads(reads), expected)
    b.set_build_piece(1000)
    assert np.array_equal(b.build_from_reads(reads), expected)


# ---- the sort's loop over tiles (csrc/radix_sort.hip): MSBWT_SORT_GRID caps its grids, so a workgroup takes several tiles ----

@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("grid", [1, 7])  # plain_100: 404 000 suffixes, 99 tiles -- all in one workgroup; 14 or 15 a workgroup, the last one partial
def test_sort_grid_cap_gives_the_same_bytes(monkeypatch, grid, wide):
    reads, expected = read_set("plain_100")
    assert -(-(reads[0].size + reads[1].size - 1) // msbwt.build_reads_sort_tile()) == 99
    monkeypatch.setenv("MSBWT_SORT_GRID", str(grid))
    if wide:
        monkeypatch.setenv("MSBWT_BUILD_WIDE", "1")
    b = msbwt.RleBWT(device=0)
    assert np.array_equal(b.build_from_reads(reads), expected)
    assert b.build_stage_ms()["pieces"] == 1


def test_sort_grid_cap_over_many_small_pieces(monkeypatch):
    reads, expected = read_set("plain_100")
    monkeypatch.setenv("MSBWT_SORT_GRID", "1")
    b = msbwt.RleBWT(device=0)
    b.set_build_piece(1000)  # most pieces below one tile, the large bins a few tiles
    assert np.array_equal(b.build_from_reads(reads), expected)
    assert b.build_stage_ms()["pieces"] > 100


@pytest.mark.parametrize("value", ["0", "abc"])
def test_sort_grid_cap_that_does_not_parse_is_no_cap(monkeypatch, value):
    reads, expected = read_set("plain_100")
    monkeypatch.delenv("MSBWT_SORT_GRID", raising=False)
    b = msbwt.RleBWT(device=0)
    unset = b.build_from_reads(reads)
    monkeypatch.setenv("MSBWT_SORT_GRID", value)
    assert np.array_equal(b.build_from_reads(reads), unset) and np.array_equal(unset, expected)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_suffix_counts_at_the_tile_border(bwt, delta):
    import synth
    tile = msbwt.build_reads_sort_tile()
    want = tile + delta  # suffixes = symbols + reads
    rng = np.random.default_rng(50 + delta)
    lengths = []
    while sum(lengths) + len(lengths) < want - 60:
        lengths.append(int(rng.integers(0, 58)))
    lengths.append(want - sum(lengths) - len(lengths) - 1)
    reads = [np.array([1, 2, 3, 5, 4], dtype=np.uint8)[rng.choice(5, size=n, p=[0.3, 0.2, 0.2, 0.25, 0.05])] for n in lengths]
    assert sum(lengths) + len(lengths) == want
    expected = synth.rle_encode(synth.build_msbwt_symbols(reads, 2))
    assert np.array_equal(bwt.build_from_reads(reads), expected)


# ---- long runs ----

def digits(rle):
    return [(int(b) & 7, int(b) >> 3) for b in rle]


def test_runs_of_exactly_32(bwt, orc):
    got = bwt.build_from_reads(["A"] * 32, ascii=True)   # BWT = 32 x 'A', then 32 x '$'
    assert digits(got) == [(1, 0), (1, 1), (0, 0), (0, 1)]
    assert np.array_equal(got, naive_rle(orc, ["A"] * 32))


def test_runs_of_exactly_1024(bwt, orc):
    got = bwt.build_from_reads(["A"] * 1024, ascii=True)
    assert digits(got) == [(1, 0), (1, 0), (1, 1), (0, 0), (0, 0), (0, 1)]
    assert np.array_equal(got, orc.convert_to_vec("A" * 1024 + "$" * 1024))


def test_runs_beyond_1024(bwt):
    import synth
    reads = ["AAA"] * 1100 + ["AAC", "GAAA", "T", "", "AAAA"]
    codes = [msbwt.string_util.convert_stoi(r) for r in reads]
    expected = synth.rle_encode(synth.build_msbwt_symbols(codes, 2))
    got = bwt.build_from_reads(reads, ascii=True)
    assert np.array_equal(got, expected)
    d = digits(got)  # three digits of one symbol in a row: a run of 1024 or more
    assert any(d[i][0] == d[i + 1][0] == d[i + 2][0] for i in range(len(d) - 2))


# ---- ASCII ----

def test_ascii_mode_equals_the_codes_path(bwt):
    reads = [b"ACgtRn.acGTTT", b"acgtNNACGT", b"RRRR....", b"", b"tTtTaAcCgG-*"]
    codes = [msbwt.string_util.convert_stoi(r) for r in reads]
    assert np.array_equal(bwt.build_from_reads(reads, ascii=True), bwt.build_from_reads(codes, ascii=False))


# ---- load_reads ----

def test_load_reads_answers_like_the_oracle(orc):
    reads = ragged_set(11) + ragged_set(12) + ragged_set(13)
    rle = naive_rle(orc, reads)
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    rng = np.random.default_rng(2)
    long_enough = [orc.convert_stoi(r) for r in reads if len(r) >= 31]
    assert long_enough
    picks = [long_enough[int(i)] for i in rng.integers(0, len(long_enough), size=2000)]
    derived = np.stack([r[s:s + 31] for r, s in ((r, int(rng.integers(0, len(r) - 30))) for r in picks)])
    random31 = np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=(2000, 31))]
    kmers = np.concatenate([derived, random31])
    want = ref.count_kmers(kmers)
    assert int((want > 0).sum()) >= 2000
    built = msbwt.RleBWT(device=0)
    built.load_reads(reads, ascii=True)
    loaded = msbwt.RleBWT(device=0)
    loaded.load_vector(built.build_from_reads(reads, ascii=True))
    for b in (built, loaded):
        assert b.get_total_size() == ref.get_total_size() == sum(len(r) + 1 for r in reads)
        assert [b.get_symbol_count(s) for s in range(6)] == [ref.get_symbol_count(s) for s in range(6)]
        assert np.array_equal(b.count_kmers(kmers), want)


# ---- errors ----

def _raw_build(handle, flat, offsets, ascii, out, cap):
    length = C.c_uint64(0)
    rc = _lib.lib().msbwt_rle_build_from_reads(handle, flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), offsets.size - 1, ascii,
                                               out.ctypes.data_as(C.c_void_p), cap, C.byref(length))
    return rc, length.value


def test_errors_leave_the_handle_usable(bwt, orc):
    for reads, ascii in (([bytes([1, 2, 0, 3])], False), ([bytes([1, 6])], False), (["AC$GT"], True)):
        with pytest.raises(msbwt.MsbwtError) as err:
            bwt.build_from_reads(reads, ascii=ascii)
        assert err.value.code == _lib.ERR_INVALID_SYMBOL
    reads = ragged_set(21)
    expected = naive_rle(orc, reads)
    flat, offsets = msbwt.rle_bwt.pack_reads(reads, ascii=True)
    out = np.full(expected.size + 8, 0xAB, dtype=np.uint8)
    rc, need = _raw_build(bwt._h, flat, offsets, 1, out, expected.size - 1)
    assert rc == _lib.ERR_INVALID_ARG and need == expected.size
    assert (out == 0xAB).all()
    rc, need = _raw_build(bwt._h, flat, offsets, 1, out, expected.size)
    assert rc == 0 and need == expected.size and np.array_equal(out[:need], expected) and (out[need:] == 0xAB).all()
