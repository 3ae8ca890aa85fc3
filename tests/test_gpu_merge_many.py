"""The one-pass merge of any number of BWTs (csrc/merge_many.hip) against the builders of the tree: the merge of the BWTs of several
read sets is the BWT of their union, so oracle.naive_bwt, synth.build_msbwt_symbols + synth.rle_encode and closed forms give the
expected bytes; they never come from the merge itself.  The expected sources (for every merged row, the input it came from) come
from a numpy restatement of the iteration in this file -- a stable argsort of the source array by the symbol each row reads, until
nothing changes -- which one test checks against a fold of the two-input merge's interleave.

Shapes: the smallest at which each mechanism can fail -- 2, 3, 5, 8 and 32 inputs (one, two and eight words of packed counts), an
empty input and an input of one empty read, merged totals at the tile's borders with whole tiles from one input and with all 32
inputs in every tile, runs that cross 32, 1024 and 2^20 symbols only once merged, and one closed-form case beyond 2^32 rows."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest

from test_gpu_merge import border_case, homopolymer_runs, reads_of  # noqa: F401  (reads_of: border_case's generator)
from test_gpu_reads_build import naive_rle, ragged_set, read_set

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
rle_decode, rle_total = msbwt.rle_bwt.rle_decode, msbwt.rle_bwt.rle_total
EMPTY = np.empty(0, dtype=np.uint8)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def bwt():
    return msbwt.RleBWT(device=0)


def expected_sources(rles):
    """The iteration, restated: the rows of input 0, then 1, and so on; every step is a stable sort of that array by the symbol each
    row reads (the rows of one input read its symbols in order)."""
    codes = [rle_decode(r) for r in rles]
    src = np.concatenate([np.full(c.size, i, dtype=np.uint8) for i, c in enumerate(codes)] + [EMPTY])
    for _ in range(src.size + 2):
        syms = np.empty(src.size, dtype=np.uint8)
        for i, c in enumerate(codes):
            syms[src == i] = c
        nxt = src[np.argsort(syms, kind="stable")]
        if np.array_equal(nxt, src):
            return src
        src = nxt
    raise AssertionError("the restated iteration did not settle")


def check_sources(sources, merged, rles):
    """The rows of source i, in order, are input i."""
    rows = rle_decode(merged)
    assert sources.dtype == np.uint8 and sources.size == rows.size
    for i, r in enumerate(rles):
        assert np.array_equal(rows[sources == i], rle_decode(r)), i
    assert int(sources.max(initial=0)) < max(len(rles), 1)


# ---- the reference's fold case, the tie rule, two inputs ----

def test_reference_fold_case_in_one_call(bwt, orc):
    strings = ["A", "AA", "AAA", "AAAA", "AAAAA"]
    want = orc.convert_to_vec(orc.naive_bwt(strings))
    for order in (strings, strings[::-1]):
        rles = [naive_rle(orc, [s]) for s in order]
        fold = rles[0]
        for r in rles[1:]:
            fold = bwt.merge(fold, r)
        got, sources = bwt.merge_many(rles, return_sources=True)
        assert np.array_equal(got, want)
        assert np.array_equal(got, fold)
        check_sources(sources, got, rles)
        assert msbwt.bwt_util.multi_bwt_merge([orc.naive_bwt([s]) for s in order], device=0) == orc.naive_bwt(strings)


def test_equal_rotations_keep_input_order(bwt, orc):
    rles = [naive_rle(orc, ["A"] * 3), naive_rle(orc, ["A"] * 2), naive_rle(orc, ["A"])]
    merged, sources = bwt.merge_many(rles, return_sources=True)
    assert np.array_equal(merged, naive_rle(orc, ["A"] * 6))
    assert sources.tolist() == [0, 0, 0, 1, 1, 2] * 2  # the '$' block, then the 'A' block


@pytest.mark.parametrize("seed", range(5))
def test_two_inputs_are_the_pairwise_merge(bwt, orc, seed):
    a = ragged_set(seed)
    b = ragged_set(100 + seed) + [a[0], a[-1]]
    ra, rb = naive_rle(orc, a), naive_rle(orc, b)
    pair, bits = bwt.merge(ra, rb, return_interleave=True)
    many, sources = bwt.merge_many([ra, rb], return_sources=True)
    assert np.array_equal(pair, naive_rle(orc, a + b))
    assert np.array_equal(many, pair)
    assert np.array_equal(sources, bits)


def test_restated_iteration_is_a_fold_of_the_pairwise_interleave(bwt, orc):
    """The source array the numpy restatement gives is the one a left fold of the two-input merge's interleave gives."""
    sets = [ragged_set(40), ragged_set(41) + ragged_set(40)[:3], [""], ragged_set(42), ragged_set(40)[-2:]]
    rles = [naive_rle(orc, s) for s in sets]
    folded, sources = rles[0], np.zeros(rle_total(rles[0]), dtype=np.uint8)
    for i, r in enumerate(rles[1:], start=1):
        folded, bits = bwt.merge(folded, r, return_interleave=True)
        grown = np.full(bits.size, i, dtype=np.uint8)
        grown[bits == 0] = sources
        sources = grown
    assert np.array_equal(folded, naive_rle(orc, sum(sets, [])))
    assert np.array_equal(expected_sources(rles), sources)


# ---- ragged collections ----

def ragged_collection(n, seed):
    """n read sets: ragged ones with reads repeated across them, an empty set in the middle, a set of one empty read."""
    rng = np.random.default_rng(7000 + 100 * n + seed)
    size = 40 if n <= 8 else 8  # (reads per set at the most: the union stays a few thousand symbols)
    sets = [ragged_set(300 * n + 10 * seed + i)[:size] for i in range(n)]
    for i in range(1, n):
        donor = sets[int(rng.integers(0, i))]
        sets[i] = sets[i] + [donor[int(rng.integers(0, len(donor)))], donor[0][:int(rng.integers(0, 9))]]
    sets[n // 2] = []
    sets[n - 2 if n > 3 else 0] = [""]
    return sets


@pytest.mark.parametrize("n,seed", [(n, s) for n in (3, 5, 8) for s in range(10)] + [(32, s) for s in range(3)])
def test_ragged_collections(bwt, orc, n, seed):
    sets = ragged_collection(n, seed)
    assert len(sets) == n and [] in sets and [""] in sets
    rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
    want = naive_rle(orc, sum(sets, []))
    got, sources = bwt.merge_many(rles, return_sources=True)
    assert np.array_equal(got, want)
    assert np.array_equal(sources, expected_sources(rles))
    check_sources(sources, got, rles)
    assert np.array_equal(bwt.merge_many(rles[::-1]), want)


# ---- tile borders ----

def cut_reads(reads, split):
    if split == "first":
        return [reads[:-2], reads[-2:-1], reads[-1:]]  # whole tiles come from one input
    if split == "last":
        return [reads[:1], reads[1:2], reads[2:]]
    if split == "even":
        return [reads[:len(reads) // 3], reads[len(reads) // 3:2 * len(reads) // 3], reads[2 * len(reads) // 3:]]
    return [reads[i::32] for i in range(32)]  # round robin: rows of all 32 inputs everywhere


@pytest.mark.parametrize("split", ["first", "last", "even", "round robin over 32"])
@pytest.mark.parametrize("delta", [-1, 0, 1, "two tiles and a row"])
def test_totals_at_the_tile_border(bwt, delta, split):
    tile = msbwt.merge_tile()
    want = 2 * tile + 1 if isinstance(delta, str) else tile + delta
    reads, expected = border_case(want)
    parts = cut_reads(reads, split)
    assert sum(len(p) for p in parts) == len(reads) and all(parts)
    rles = [bwt.build_from_reads(p) for p in parts]
    assert sum(rle_total(r) for r in rles) == want
    wanted_sources = expected_sources(rles)
    if len(parts) == 32:  # every tile holds rows of all 32 inputs (but a last tile of one row, which cannot)
        for lo in range(0, want, tile):
            assert np.unique(wanted_sources[lo:lo + tile]).size == 32 or want - lo == 1
    merged, sources = bwt.merge_many(rles, return_sources=True)
    assert np.array_equal(merged, expected)
    assert np.array_equal(sources, wanted_sources)
    check_sources(sources, merged, rles)


# ---- one input ----

def _raw_merge_many(handle, rles, out, cap, sources=None):
    flat, offsets = msbwt.rle_bwt._pack_rles(rles)
    length = C.c_uint64(0)
    rc = _lib.lib().msbwt_rle_merge_many(handle, flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), len(rles), out.ctypes.data_as(C.c_void_p), cap,
                                         C.byref(length), None if sources is None else sources.ctypes.data_as(C.c_void_p))
    return rc, length.value


def test_one_input_that_is_not_canonical_comes_back_canonical(bwt, orc):
    # 1100 'A' as 600 and 500 with an empty '$' run between the two byte groups, 1100 '$' as 76 + 32 * 32 with two empty digits on top
    loose = np.array([1 | 24 << 3, 1 | 18 << 3, 0, 1 | 20 << 3, 1 | 15 << 3, 0 | 12 << 3, 0 | 2 << 3, 0 | 1 << 3, 0, 0], dtype=np.uint8)
    want = orc.convert_to_vec("A" * 1100 + "$" * 1100)
    assert want.size == 6 and rle_total(loose) == 2200
    got, sources = bwt.merge_many([loose], return_sources=True)
    assert np.array_equal(got, want)
    assert sources.size == 2200 and not sources.any()
    assert bwt.merge_info()["iterations"] >= 1
    out = np.full(want.size + 8, 0xAB, dtype=np.uint8)
    rc, need = _raw_merge_many(bwt._h, [loose], out, want.size - 1)
    assert rc == _lib.ERR_INVALID_ARG and need == want.size
    assert (out == 0xAB).all()
    rc, need = _raw_merge_many(bwt._h, [loose], out, want.size)
    assert rc == 0 and need == want.size and np.array_equal(out[:need], want) and (out[need:] == 0xAB).all()


# ---- the inputs' places in the one array of RLE bytes ----

def trimmed_to(orc, reads, residue):
    """`reads` with letters taken off their ends, one at a time, until their BWT takes `residue` RLE bytes modulo 16."""
    reads = list(reads)
    for step in range(200):
        if naive_rle(orc, reads).size % 16 == residue:
            return reads
        longest = max(range(len(reads)), key=lambda i: len(reads[i]))
        reads[longest] = reads[longest][:-1]
    raise AssertionError("no trim of the read set takes %d bytes modulo 16" % residue)


def test_inputs_whose_rle_bytes_end_off_a_16_byte_border(bwt, orc):
    """The inputs' RLE bytes lie one after the other in HBM, each at a 16-byte border (the decoder loads 16 bytes at a time):
    three inputs of 1, 0 and 15 bytes modulo 16, and one of no bytes between two of them."""
    sets = [trimmed_to(orc, ragged_set(seed), residue) for seed, residue in ((300, 1), (302, 0), (303, 15))]
    rles = [naive_rle(orc, reads) for reads in sets]
    assert [r.size % 16 for r in rles] == [1, 0, 15] and all(r.size > 16 for r in rles)
    rles.insert(1, EMPTY)
    merged, sources = bwt.merge_many(rles, return_sources=True)
    assert np.array_equal(merged, bwt.build_from_reads(sets[0] + sets[1] + sets[2], ascii=True))
    assert np.array_equal(merged, naive_rle(orc, sets[0] + sets[1] + sets[2]))
    assert np.array_equal(sources, expected_sources(rles))
    check_sources(sources, merged, rles)


# ---- convergence ----

def test_convergence_takes_longer_than_the_read_length(bwt, orc):
    rng = np.random.default_rng(9)
    read = "".join(rng.choice(list("ACGT"), size=60))
    others = [read[:59] + c for c in "ACGTN" if c != read[59]]
    sets = [[read] * 30 + others[:2] + [read[:59]], [read] * 30 + others[2:3] + [read[:30]], [read] * 20 + others[3:]]
    rles = [naive_rle(orc, s) for s in sets]
    merged = bwt.merge_many(rles)
    assert bwt.merge_info()["iterations"] > 61  # rotations of the repeated read are told apart only after a whole turn
    assert np.array_equal(merged, naive_rle(orc, sum(sets, [])))


# ---- runs ----

def homopolymer_rle(counts, length, path):
    msbwt.bwt_converter.save_bwt_runs_numpy(homopolymer_runs(counts, length), path)
    return np.array(np.load(path))


def homopolymer_sources(inputs, length):
    """The source array of the merge of homopolymer inputs: within a group of equal rotations, input order.  The '$' block has one
    group per letter, a letter's block `length` groups."""
    group = lambda c: np.repeat(np.arange(len(inputs), dtype=np.uint8), [counts.get(c, 0) for counts in inputs])
    return np.concatenate([group(c) for c in "ACGNT"] + [np.tile(group(c), length) for c in "ACGNT"])


def test_runs_that_cross_the_digit_borders_once_merged(bwt, orc, tmp_path):
    length = 3
    inputs = [{"A": 400000, "C": 400, "G": 12}, {"A": 300000, "C": 300, "G": 9, "T": 7}, {"A": 200000, "C": 200, "G": 6}]
    both = {c: sum(counts.get(c, 0) for counts in inputs) for c in "ACGNT"}
    for c, border in (("G", 32), ("C", 1024), ("A", 2 ** 20)):  # the letter's run before its '$'s: below the border in every input, above it merged
        assert all(counts[c] * (length - 1) < border for counts in inputs) and both[c] * (length - 1) > border
    small = [{"A": 3, "C": 2}, {"A": 1, "T": 2}, {"C": 1, "T": 1}]  # the closed forms themselves, against naive_bwt
    reads = lambda counts: [c * length for c in "ACGNT" for _ in range(counts.get(c, 0))]
    text = lambda runs: "".join("$ACGNT"[s] * n for s, n in runs)
    assert text(homopolymer_runs({"A": 4, "C": 3, "T": 3}, length)) == orc.naive_bwt(sum((reads(s) for s in small), []))
    assert np.array_equal(homopolymer_sources(small, length), expected_sources([naive_rle(orc, reads(s)) for s in small]))
    rles = [homopolymer_rle(counts, length, str(tmp_path / ("in%d.npy" % i))) for i, counts in enumerate(inputs)]
    want = homopolymer_rle(both, length, str(tmp_path / "both.npy"))
    got, sources = bwt.merge_many(rles, return_sources=True)
    assert np.array_equal(got, want)
    assert np.array_equal(sources, homopolymer_sources(inputs, length))


# ---- beyond 2^32 rows ----

def test_beyond_2_to_32_rows(tmp_path):
    """4.41e9 merged rows from three inputs of a few dozen RLE bytes; read length 29, 30 iterations.  Measured on an MI355X: the merge
    call takes 0.92 s (iterate 0.61 s, the 4.4 GB of sources to the host 0.28 s) and the checks after it 0.15 s, so the read length
    stays at 29; where this test is the first of its process to start torch, that start-up adds about 13 s before the call."""
    started = time.perf_counter()
    import torch
    length = 29
    inputs = [{"A": 5 * 10 ** 7, "C": 3 * 10 ** 7, "T": 10 ** 7}, {"A": 2 * 10 ** 7, "G": 2 * 10 ** 7, "T": 10 ** 7}, {"C": 4 * 10 ** 6, "N": 3 * 10 ** 6}]
    both = {c: sum(counts.get(c, 0) for counts in inputs) for c in "ACGNT"}
    totals = [sum(counts.values()) * (length + 1) for counts in inputs]
    total = sum(totals)
    assert total == 441 * 10 ** 7 > 2 ** 32
    need = msbwt.merge_many_plan(totals)
    free, _ = torch.cuda.mem_get_info(0)
    if free < need + need // 4:
        pytest.skip("%.1f GB of HBM free, the merge takes %.1f GB" % (free / 1e9, need / 1e9))
    rles = [homopolymer_rle(counts, length, str(tmp_path / ("in%d.npy" % i))) for i, counts in enumerate(inputs)]
    want = homopolymer_rle(both, length, str(tmp_path / "both.npy"))
    assert [rle_total(r) for r in rles] == totals and rle_total(want) == total
    b = msbwt.RleBWT(device=0)
    out = np.zeros(sum(r.size for r in rles), dtype=np.uint8)
    sources = np.empty(total, dtype=np.uint8)
    t0 = time.perf_counter()
    rc, got = _raw_merge_many(b._h, rles, out, out.size, sources)
    print("merge of %d rows: %.2f s after %.2f s of set-up, %s" % (total, time.perf_counter() - t0, t0 - started, b.merge_info()))
    assert rc == 0, _lib.lib().msbwt_rle_last_error(b._h)
    assert np.array_equal(out[:got], want)
    source_at = lambda group, k: int(np.searchsorted(np.cumsum(group), k, side="right"))  # the input of row k of a group of equal rotations
    borders = {}  # row -> the input it came from
    at = 0
    blocks = [(c, 1) for c in "ACGNT"] + [(c, length) for c in "ACGNT"]  # the '$' block's groups, then the letters' blocks
    tail_from = 2 ** 32 - 2 * 10 ** 8
    tail_counts = np.zeros(len(inputs), dtype=np.int64)
    for c, groups in blocks:
        group = [counts.get(c, 0) for counts in inputs]
        size = sum(group)
        for g in range(groups if size else 0):
            lo = at + g * size
            if groups == 1 or lo + size > tail_from:  # every '$' group, and the groups around row 2^32 and after it
                ends = np.cumsum(group)
                for k in [0, size - 1] + [int(e) + d for e in ends[:-1] for d in (-1, 0)] + [r - lo for r in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)]:
                    if 0 <= k < size:
                        borders[lo + k] = source_at(group, k)
            for i, n in enumerate(group):  # rows of input i from tail_from on
                first = lo + sum(group[:i])
                tail_counts[i] += max(0, first + n - max(first, tail_from))
        at += size * groups
    assert at == total and any(r > 2 ** 32 for r in borders) and {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1} <= set(borders)
    for row, want_source in sorted(borders.items()):
        assert int(sources[row]) == want_source, row
    tail = sources[tail_from:]
    assert [int(np.count_nonzero(tail == i)) for i in range(len(inputs))] == tail_counts.tolist()
    assert b.merge_info()["iterations"] >= length
    print("checks done %.2f s after the start" % (time.perf_counter() - started))


# ---- loading the merged BWT ----

def test_load_merged_many(orc):
    (flat, offsets), expected = read_set("plain_100")
    n = offsets.size - 1
    b = msbwt.RleBWT(device=0)
    b.load_vector(orc.convert_to_vec(orc.naive_bwt(["ACGT", "CCGT"])))  # an index the merge has to release
    assert b.get_total_size() == 10
    cuts = [0, n // 4, n // 4 + n // 3, n]
    rles = [b.build_from_reads((flat, offsets[lo:hi + 1])) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert b.get_total_size() == 10
    b.load_merged_many(rles)
    ref = msbwt.RleBWT(device=0)
    ref.load_vector(expected)
    assert b.get_total_size() == ref.get_total_size() == rle_total(expected)
    assert [b.get_symbol_count(s) for s in range(6)] == [ref.get_symbol_count(s) for s in range(6)]
    rng = np.random.default_rng(3)
    length = int(offsets[1])
    reads = flat.reshape(n, length)
    rows, starts = rng.integers(0, n, size=2000), rng.integers(0, length - 30, size=2000)
    kmers = np.ascontiguousarray(np.stack([reads[r, s:s + 31] for r, s in zip(rows, starts)]))
    want = ref.count_kmers(kmers)
    assert int(want.min()) >= 1
    assert np.array_equal(b.count_kmers(kmers), want)
    b.load_merged_many(rles[:2])  # and the handle is used again
    assert b.get_total_size() == rle_total(rles[0]) + rle_total(rles[1])


def test_merge_numpy_files_gives_the_same_file_either_way(orc, tmp_path):
    sets = [ragged_set(60 + i) for i in range(5)]
    paths = []
    for i, s in enumerate(sets):
        paths.append(str(tmp_path / ("in%d.npy" % i)))
        msbwt.bwt_converter.save_bwt_numpy(naive_rle(orc, s), paths[-1])
    tree, one = str(tmp_path / "tree.npy"), str(tmp_path / "one.npy")
    msbwt.bwt_util.merge_numpy_files(paths, tree, device=0, method="tree")
    msbwt.bwt_util.merge_numpy_files(paths, one, device=0, method="one_pass")
    assert open(tree, "rb").read() == open(one, "rb").read()
    auto = str(tmp_path / "auto.npy")
    assert len(paths) >= msbwt.bwt_util.ONE_PASS_MIN_INPUTS  # so "auto" takes the one pass
    msbwt.bwt_util.merge_numpy_files(paths, auto, device=0)
    assert open(auto, "rb").read() == open(tree, "rb").read()
    assert np.array_equal(np.load(one), naive_rle(orc, sum(sets, [])))
    with pytest.raises(ValueError):
        msbwt.bwt_util.merge_numpy_files(paths * 7, one, device=0, method="one_pass")
