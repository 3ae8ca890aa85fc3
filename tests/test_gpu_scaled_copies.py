"""The producers and what hangs off them beyond 2^32 rows on real reads: the builder from reads (csrc/reads_build.hip), the two merges
(csrc/merge.hip, csrc/merge_many.hip), the source index (csrc/source_index.hip) and the k-mer enumeration (csrc/spectrum.hip).

Every index here is S x c: a ragged read set S of about 10^6 rows (reads of 0..41 symbols over ACGTN, duplicates, prefixes, empty
reads, reads shared between the inputs of a merge) with every read c = 4096 or 4369 times.  Row for row its BWT, the source vector
of its merges and its k-mer ranges are those of S with every row repeated c times (tests/test_scaled_copies.py proves that on the
CPU and holds the helpers), so every expected value comes from the CPU builder synth.build_msbwt_symbols, the restated merge
iteration test_gpu_merge_many.expected_sources, a numpy census of the reads' windows and the CPU oracle on S -- never from the code
under test.  Unlike the homopolymer cases of the neighbouring files these indexes scatter their rows: an LF step moves a row across
the whole index, a truncated position lands in another read, there are 2.9e5 distinct 12-mers and the ranges of a k-mer's copies
lie on both sides of row 2^32 all over the index.

Totals: 2^32 - 1 (the last text the builder sorts with 32-bit positions), 2^32 (the first with 64-bit ones) and 4 505 600 000.

Measured on a free MI355X (308 GB of HBM, none of the cases skipped; every gate prints what was free and what it needed when it
does skip).  The builder's automatic piece was 8.1e9 suffixes, so each text was sorted as one piece:

* narrow limit: 201 166 236 reads, 4 294 967 295 symbols, 1 piece, 2 214 039 RLE bytes; the build 3.9 s as the first of its
  process (sort 0.66 s; 2.5 s of it the first allocation of the sort buffers, booked under `collect`), the test 6.2 s;
* past it: 211 025 920 reads, 4 505 600 000 symbols, 1 piece, 2 476 649 RLE bytes, 4.5 s (sort 0.71 s); again under a piece limit
  of 10^9 suffixes: 5 pieces, 1.3 to 5.5 s; the test 10.8 s;
* wide first: 201 134 080 reads, 4 294 967 296 symbols, 1 piece, 2 360 810 RLE bytes, 1.3 s (sort 0.73 s), the test 2.1 s (4.8 s in
  a run of the whole suite, where the buffers were not at hand);
* load_reads of the 4 505 600 000 symbols into run blocks 5.0 s, 2000 of the 4000 31-mers present, the test 5.1 to 5.6 s;
* the merge of two: 0.7 to 0.8 s (18 iterations, iterate 0.27 s), the word compare of the 4.5e9 interleave entries 0.6 s, the test
  with its CPU expectation 5.8 s;
* the merge of three: 0.7 s (19 iterations, iterate 0.40 s, the 4.5 GB of sources to the host 0.27 s), the compare 0.5 s;
* its index: load_merged_many with the sources kept 1.3 s, every k-mer call of k = 12 (293 181 k-mers, the widest range 20 480 rows,
  17 440 ranges start past row 2^32, one straddles it) and k = 31 (16 354 k-mers, 984 past, one astride) 0.13 s together, the
  narrow ranges 0.00 s; the three merge tests with the CPU expectations of both cases 8.4 to 9.1 s.

The whole file takes 36 s.  With `Pos(uint32_t(base + i))` stored in k_piece_collect<uint64_t> (a
library built apart for that, not kept) "past it" fails -- 2 395 487 RLE bytes for 2 476 649 -- and "narrow limit" passes.
"""
import importlib
import time

import numpy as np
import pytest

from test_gpu_merge_many import expected_sources
from test_gpu_sparse import oracle_ranges
from test_scaled_copies import CODES, EMPTY, U64, bwt_symbols, census_of_codes, copy_set, counts_in, first_row_that_is_not_repeated, random_reads, scaled_rle, tiled

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
rle_total, unpack_2bit = msbwt.rle_bwt.rle_total, msbwt.rle_bwt.unpack_2bit
EDGE = 2 ** 32
COPIES = 4096
SMALL_EDGE = EDGE // COPIES  # row 2^32 is the first copy of this row of the small index
BUILDS = {"narrow limit": (983055, 4369), "wide first": (1048576, 4096), "past it": (1100000, 4096)}  # rows of S, c
# The third input of the merge of three ends with LIFT reads TTT and four empty reads for each of the 400 - LIFT others.  A read TTT
# puts three rows below row 2^20 of the small union and one (TTT$) above it, four empty reads put four below: LIFT chooses, row by
# row, which suffix of the union sits at row 2^20.  92 (found on the CPU, by the oracle's ranges on the small union) puts a 12-mer
# and a 31-mer that occur twice there, so that their ranges on the GPU straddle row 2^32; the test asserts that they do.
LIFT, LIFT_ROOM = 92, 400


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def free_or_skip(what, need):
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        print("%s: %.1f GB of HBM free, %.1f GB needed" % (what, free / 1e9, need / 1e9))
        pytest.skip("%s: %.1f GB of HBM free, %.1f GB needed" % (what, free / 1e9, need / 1e9))
    return free


def rle_of(symbols):
    import synth
    return synth.rle_encode(symbols)


# ---- 1. the builder at the border of its two instantiations ----

_sets = {}


def small_set(rows):
    """(reads, the CPU builder's BWT symbols of them), computed once per row count."""
    if rows not in _sets:
        reads = copy_set(rows, 11)
        symbols = bwt_symbols(reads)
        symbols.setflags(write=False)
        _sets[rows] = (reads, symbols)
    return _sets[rows]


def build_need(total, free):
    need = msbwt.build_reads_plan(total, free, 10 ** 9)[1]
    return need + need // 4


@pytest.mark.parametrize("case", sorted(BUILDS))
def test_builder_at_the_border_of_its_two_instantiations(case, tmp_path):
    started = time.perf_counter()
    rows, c = BUILDS[case]
    total = rows * c
    assert {"narrow limit": total == EDGE - 1, "wide first": total == EDGE, "past it": total == 4505600000 > EDGE}[case]
    import torch
    free = free_or_skip("build of %d symbols" % total, build_need(total, torch.cuda.mem_get_info(0)[0]))
    reads, symbols = small_set(rows)
    want = scaled_rle(symbols, c, str(tmp_path / "want.npy"))
    assert rle_total(want) == total
    flat, offsets = tiled(reads, c)
    assert int(offsets[-1]) + offsets.size - 1 == total and int(offsets[len(reads)]) - int(offsets[0]) == flat.size // c
    b = msbwt.RleBWT(device=0)
    auto_piece = msbwt.build_reads_plan(total, free, 0)[0]
    t0 = time.perf_counter()
    got = b.build_from_reads((flat, offsets))
    t1 = time.perf_counter()
    first = b.build_stage_ms()
    print("%s: %d reads, %d symbols, %d pieces (automatic piece %d), %d RLE bytes: %.2f s after %.2f s of set-up; %s"
          % (case, offsets.size - 1, total, first["pieces"], auto_piece, got.size, t1 - t0, t0 - started, {k: round(v) for k, v in first.items()}))
    second = None
    if case == "past it":
        b.set_build_piece(10 ** 9)
        again = b.build_from_reads((flat, offsets))
        second = b.build_stage_ms()
        print("%s under a piece limit of 10^9: %d pieces, %.2f s" % (case, second["pieces"], time.perf_counter() - t1))
    del flat, offsets
    assert np.array_equal(got, want), (got.size, want.size)
    assert first["pieces"] == 1 or auto_piece < total + total // 8  # one piece wherever the automatic limit is well above the total
    if second is not None:
        assert second["pieces"] > 1 and second["pieces"] >= total // 10 ** 9
        assert np.array_equal(again, got) and np.array_equal(again, want)
    print("%s: %.2f s in all" % (case, time.perf_counter() - started))


# ---- 2. load_reads ----

def test_load_reads_past_2_to_32(orc):
    started = time.perf_counter()
    rows, c = BUILDS["past it"]
    total = rows * c
    assert total > EDGE
    free_or_skip("load_reads of %d symbols" % total, 8 * total)
    reads, symbols = small_set(rows)
    ref = orc.OracleRleBWT()
    ref.load_vector(rle_of(symbols))
    rng = np.random.default_rng(31)
    long_enough = [r for r in reads if r.size >= 31]
    picks = [long_enough[int(i)] for i in rng.integers(0, len(long_enough), size=2000)]
    windows = np.stack([r[s:s + 31] for r, s in ((r, int(rng.integers(0, r.size - 30))) for r in picks)])
    kmers = np.ascontiguousarray(np.concatenate([windows, CODES[:4][rng.integers(0, 4, size=(2000, 31))]]))
    want = ref.count_kmers(kmers) * U64(c)
    assert int((want > 0).sum()) >= 1000
    flat, offsets = tiled(reads, c)
    b = msbwt.RleBWT(device=0)
    b.set_block_format("runs")  # the lean index: 4.5e9 rows of it load faster than planes and a pair index
    t0 = time.perf_counter()
    b.load_reads((flat, offsets))
    t1 = time.perf_counter()
    del flat, offsets
    assert b.get_block_format() == "runs"
    assert b.get_total_size() == c * ref.get_total_size() == total
    assert [b.get_symbol_count(s) for s in range(6)] == [c * ref.get_symbol_count(s) for s in range(6)]
    got = b.count_kmers(kmers)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    print("load_reads of %d symbols: %.2f s after %.2f s of set-up, %d of %d 31-mers present, %.2f s in all"
          % (total, t1 - t0, t0 - started, int((want > 0).sum()), len(kmers), time.perf_counter() - started))


# ---- 3. the merge of two ----

_pair = {}


def pair_case():
    """S0 of 600 000 and S1 of 500 000 rows that share 200 reads: their BWTs' symbols, those of the union, the expected interleave."""
    if not _pair:
        shared = random_reads(np.random.default_rng(20), np.random.default_rng(21).integers(0, 42, size=200))
        sets = [copy_set(600000, 22, shared), copy_set(500000, 23, shared)]
        symbols = [bwt_symbols(s) for s in sets]
        _pair.update(symbols=symbols, union=bwt_symbols(sets[0] + sets[1]), interleave=expected_sources([rle_of(s) for s in symbols]))
        for a in symbols + [_pair["union"], _pair["interleave"]]:
            a.setflags(write=False)
    return _pair


def test_merge_of_two_past_2_to_32(tmp_path):
    started = time.perf_counter()
    case, c = pair_case(), COPIES
    totals = [s.size * c for s in case["symbols"]]
    total = sum(totals)
    assert totals == [600000 * c, 500000 * c] and total == 4505600000 > EDGE
    need = msbwt.merge_plan(*totals)
    free_or_skip("merge of %d rows" % total, need + need // 4)
    small = case["interleave"]
    for i in (0, 1):  # both inputs have rows on both sides of row 2^32
        assert (small[:SMALL_EDGE] == i).any() and (small[SMALL_EDGE:] == i).any()
    assert np.count_nonzero(small[SMALL_EDGE + 1:] != small[SMALL_EDGE:-1]) > 1000
    rles = [scaled_rle(s, c, str(tmp_path / ("in%d.npy" % i))) for i, s in enumerate(case["symbols"])]
    want = scaled_rle(case["union"], c, str(tmp_path / "union.npy"))
    assert [rle_total(r) for r in rles] == totals and rle_total(want) == total
    b = msbwt.RleBWT(device=0)
    t0 = time.perf_counter()
    got, bits = b.merge(rles[0], rles[1], return_interleave=True)
    t1 = time.perf_counter()
    info = b.merge_info()
    ones = int(np.count_nonzero(bits)) if bits.size == total else -1
    wrong = first_row_that_is_not_repeated(bits, small, c) if bits.size == total else 0
    del bits
    print("merge of %d rows: %.2f s after %.2f s of set-up, %s; checks %.2f s" % (total, t1 - t0, t0 - started, info, time.perf_counter() - t1))
    assert np.array_equal(got, want)
    assert ones == totals[1]
    assert wrong == -1, "the copies of small row %d (its bit is %d)" % (wrong, small[wrong])


# ---- 4. the merge of three, its sources and its k-mers ----

_three = {}
KS = (12, 31)


def three_case(orc):
    """S0, S1, S2 of 500 000, 400 000 and 200 000 rows with reads shared between every pair and among all three, empty reads in all
    and more of them in S2: the symbols of their BWTs and of the union's, the expected sources, and per k the census of the union,
    of every input, and the oracle's range starts on the small union."""
    if not _three:
        rng = np.random.default_rng(4)
        clean = lambda rs: [np.where(r == 4, 1, r).astype(np.uint8) for r in rs]  # no N: their 31-mers count
        all3 = clean(random_reads(rng, [41] * 20 + [31] * 20 + [12] * 10))
        p01, p02, p12 = (clean(random_reads(rng, [41] * 10 + [20] * 10)) for _ in range(3))
        ttt = np.array([5, 5, 5], dtype=np.uint8)
        sets = [copy_set(500000, 40, all3 + p01 + p02), copy_set(400000, 41, all3 + p01 + p12),
                copy_set(200000, 42, all3 + p02 + p12 + [EMPTY] + [ttt] * LIFT + [EMPTY] * (4 * (LIFT_ROOM - LIFT)))]
        symbols = [bwt_symbols(s) for s in sets]
        everything = sets[0] + sets[1] + sets[2]
        union = bwt_symbols(everything)
        ref = orc.OracleRleBWT()
        ref.load_vector(rle_of(union))
        _three.update(symbols=symbols, union=union, sources=expected_sources([rle_of(s) for s in symbols]))
        for k in KS:
            words, counts = census_of_codes(everything, k)
            l, h = oracle_ranges(ref, unpack_2bit(words, k))
            assert np.array_equal(h - l, counts)  # (the oracle agrees with the census)
            by_input = np.stack([counts_in(words, *census_of_codes(s, k)) for s in sets], axis=1)
            assert np.array_equal(by_input.sum(axis=1, dtype=U64), counts)
            _three[k] = (words, counts, l, by_input)
    return _three


def three_totals(case, c):
    totals = [s.size * c for s in case["symbols"]]
    assert totals == [500000 * c, 400000 * c, 200000 * c] and sum(totals) == 4505600000 > EDGE
    return totals, sum(totals)


def test_merge_of_three_past_2_to_32(orc, tmp_path):
    started = time.perf_counter()
    case, c = three_case(orc), COPIES
    totals, total = three_totals(case, c)
    need = msbwt.merge_many_plan(totals)
    free_or_skip("merge of %d rows" % total, need + need // 4)
    small = case["sources"]
    for i in range(3):
        assert (small[:SMALL_EDGE] == i).any() and (small[SMALL_EDGE:] == i).any()
    rles = [scaled_rle(s, c, str(tmp_path / ("in%d.npy" % i))) for i, s in enumerate(case["symbols"])]
    want = scaled_rle(case["union"], c, str(tmp_path / "union.npy"))
    assert [rle_total(r) for r in rles] == totals and rle_total(want) == total
    b = msbwt.RleBWT(device=0)
    t0 = time.perf_counter()
    got, sources = b.merge_many(rles, return_sources=True)
    t1 = time.perf_counter()
    info = b.merge_info()
    wrong = first_row_that_is_not_repeated(sources, small, c) if sources.size == total else 0
    del sources
    print("merge of %d rows: %.2f s after %.2f s of set-up, %s; checks %.2f s" % (total, t1 - t0, t0 - started, info, time.perf_counter() - t1))
    assert np.array_equal(got, want)
    assert wrong == -1, "the copies of small row %d (its source is %d)" % (wrong, small[wrong])


def test_sources_and_kmers_of_the_merge_of_three(orc, tmp_path):
    started = time.perf_counter()
    case, c = three_case(orc), COPIES
    totals, total = three_totals(case, c)
    free_or_skip("merged index of %d rows" % total, 8 * total)
    small = case["sources"]
    rles = [scaled_rle(s, c, str(tmp_path / ("in%d.npy" % i))) for i, s in enumerate(case["symbols"])]
    b = msbwt.RleBWT(device=0)
    t0 = time.perf_counter()
    b.load_merged_many(rles, keep_sources=True)
    t1 = time.perf_counter()
    assert b.get_total_size() == total and b.source_count() == 3 and b.source_totals().tolist() == totals
    narrow = msbwt.source_narrow_rows()
    assert narrow < c
    cu = U64(c)
    for k in KS:
        words, counts, l_small, by_input = case[k]
        assert len(words) > (10 ** 5 if k == 12 else 10 ** 4) and counts.max() >= 3
        w, n, l = b.enumerate_kmers(k, ranges=True)  # (the first of them under the automatic frontier)
        b.set_spectrum_frontier(1 << 21)
        assert np.array_equal(w, words), (k, len(w), len(words))
        assert np.array_equal(n, counts * cu), (k, np.flatnonzero(n != counts * cu)[:5])
        assert np.array_equal(l, l_small * cu), (k, np.flatnonzero(l != l_small * cu)[:5])
        past, straddling = int((l > EDGE).sum()), int(((l < EDGE) & (l + n > EDGE)).sum())
        print("k = %d: %d k-mers, the largest count %d, %d ranges start past 2^32, %d straddle it" % (k, len(w), int(n.max()), past, straddling))
        # (reads of at most 41 symbols hold few 31-mers: 1.6e4 distinct ones in all, a sixteenth of them past row 2^32)
        assert past > (10 ** 4 if k == 12 else 500) and straddling >= 1
        uw, un, ul = b.enumerate_kmers(k, sorted=False, ranges=True)
        order = np.argsort(uw, kind="stable")
        assert np.array_equal(uw[order], w) and np.array_equal(un[order], n) and np.array_equal(ul[order], l), k
        keep = counts >= 2
        gw, gn = b.enumerate_kmers(k, min_count=2 * c)
        assert 0 < int(keep.sum()) < len(words) and np.array_equal(gw, words[keep]) and np.array_equal(gn, counts[keep] * cu), k
        bins = c * int(counts.max()) + 2
        hist, distinct, occurrences = b.kmer_spectrum(k, bins)
        assert np.array_equal(hist, np.bincount((counts * cu).astype(np.int64), minlength=bins).astype(U64)), k
        assert hist[bins - 1] == 0 and distinct == len(words) and occurrences == int(counts.sum()) * c
        hist, distinct, occurrences = b.kmer_spectrum(k, 256)
        assert hist[255] == len(words) and not hist[:255].any() and distinct == len(words) and occurrences == int(counts.sum()) * c
        assert (n > narrow).all()  # every range of a k-mer is c rows or more: the path through the checkpoints
        by_range = b.range_sources(l, l + n)
        for i in range(3):
            assert np.array_equal(by_range[:, i], by_input[:, i] * cu), (k, i, np.flatnonzero(by_range[:, i] != by_input[:, i] * cu)[:5])
        by_search = b.count_kmers_by_source(unpack_2bit(w, k))
        assert np.array_equal(by_search, by_range), k
        assert (by_input > 0).sum(axis=0).min() > 1000 and ((by_input > 0).sum(axis=1) == 3).sum() > 100  # every input answers, some k-mers in all
    t2 = time.perf_counter()

    # ranges inside the copies of one small row, and across the border between two small rows of different sources
    rng = np.random.default_rng(6)
    rows = np.concatenate([rng.integers(0, small.size, size=300), rng.integers(SMALL_EDGE, small.size, size=300), [SMALL_EDGE - 1, SMALL_EDGE, small.size - 1]])
    width = np.concatenate([rng.integers(1, narrow + 1, size=rows.size - 6), [1, narrow - 1, narrow, narrow, narrow + 1, c]])  # the last two: not narrow
    start = np.array([int(rng.integers(0, c - w + 1)) for w in width])
    start[-1] = 0
    l_in = rows.astype(U64) * cu + start.astype(U64)
    want_in = np.zeros((rows.size, 3), dtype=U64)
    want_in[np.arange(rows.size), small[rows]] = width
    borders = SMALL_EDGE + np.flatnonzero(small[SMALL_EDGE + 1:] != small[SMALL_EDGE:-1])  # small rows past 2^32 whose next row is another input's
    assert borders.size > 1000
    borders = borders[rng.choice(borders.size, size=300, replace=False)]
    span = np.concatenate([rng.integers(2, narrow + 1, size=borders.size - 3), [2, narrow, narrow + 1]])
    before = np.array([int(rng.integers(1, w)) for w in span])
    l_x = (borders.astype(U64) + U64(1)) * cu - before.astype(U64)
    want_x = np.zeros((borders.size, 3), dtype=U64)
    want_x[np.arange(borders.size), small[borders]] = before
    want_x[np.arange(borders.size), small[borders + 1]] = span - before
    l_all, h_all = np.concatenate([l_in, l_x]), np.concatenate([l_in + width.astype(U64), l_x + span.astype(U64)])
    asked = h_all - l_all
    assert (asked <= narrow).sum() > 500 and (asked > narrow).sum() >= 3 and (l_all > EDGE).sum() > 500 and ((l_all < EDGE) & (h_all > EDGE)).sum() == 0
    got = b.range_sources(l_all, h_all)
    assert np.array_equal(got, np.concatenate([want_in, want_x])), np.flatnonzero((got != np.concatenate([want_in, want_x])).any(axis=1))[:5]
    edge = b.range_sources(np.array([EDGE - 7, EDGE - narrow // 2], dtype=U64), np.array([EDGE + 9, EDGE + narrow // 2], dtype=U64))  # across row 2^32 itself
    want_edge = np.zeros((2, 3), dtype=U64)
    for j, (below, above) in enumerate(((7, 9), (narrow // 2, narrow // 2))):
        want_edge[j, small[SMALL_EDGE - 1]] += below
        want_edge[j, small[SMALL_EDGE]] += above
    assert np.array_equal(edge, want_edge)
    print("load_merged_many with sources, %d rows: %.2f s after %.2f s of set-up; k-mers %.2f s, narrow ranges %.2f s"
          % (total, t1 - t0, t0 - started, t2 - t1, time.perf_counter() - t2))
