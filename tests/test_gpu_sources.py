"""Counts by source (csrc/source_index.hip, csrc/sources.cpp): how often a k-mer occurs in each input of a merged BWT.

The rows of input i inside the merged range of a k-mer are exactly the occurrences of the k-mer in input i, so column i of
count_kmers_by_source equals count_kmers on input i's own BWT and the columns sum to count_kmers on the merged one.  Expected values
come from np.bincount over the source vector, from the CPU oracle on each input, and from closed forms; never from the code under
test.

Shapes: totals at the borders of a checkpoint block (R - 1, R, R + 1, 2 R + 1 rows) with 1, 2, 3, 8 and 32 sources (one checkpoint
word to two lines), ranges at the block borders and at the border between the ranges counted from their own bytes and those that go
through the checkpoints; ragged collections of 2, 3, 8 and 32 inputs with an empty input and an input of one empty read; ranges
that span thousands of blocks in closed form; and one case beyond 2^32 rows."""
import importlib
import itertools
import time

import numpy as np
import pytest

from test_gpu_merge import border_case
from test_gpu_merge_many import EMPTY, expected_sources, homopolymer_rle, ragged_collection
from test_gpu_reads_build import naive_rle, read_set

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
rle_total = msbwt.rle_bwt.rle_total
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
U64 = np.uint64


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _torch():
    import torch
    return torch


def device_range_sources(b, l, h):
    torch = _torch()
    dev = torch.device("cuda:0")
    d_l, d_h = torch.from_numpy(l.astype(np.int64)).to(dev), torch.from_numpy(h.astype(np.int64)).to(dev)
    d_out = torch.full((l.size, b.source_count()), -7, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    b.range_sources_device(d_l.data_ptr(), d_h.data_ptr(), l.size, d_out.data_ptr(), stream)
    b.device_status(stream)
    return d_out.cpu().numpy().astype(np.uint64)


def device_counts_by_source(b, kmers, check=True):
    torch = _torch()
    dev = torch.device("cuda:0")
    d_k = torch.from_numpy(np.ascontiguousarray(kmers)).to(dev)
    d_out = torch.full((kmers.shape[0], b.source_count()), -7, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    b.count_kmers_by_source_device(d_k.data_ptr(), kmers.shape[1], kmers.shape[0], d_out.data_ptr(), stream)
    if check:
        b.device_status(stream)
    else:
        torch.cuda.current_stream(dev).synchronize()
    return d_out.cpu().numpy().astype(np.uint64)


# ---- 1. checkpoint borders, against np.bincount ----

def source_patterns(total, n, rng):
    block = msbwt.source_block_rows()
    whole = np.zeros(total, dtype=np.uint8)  # whole blocks from one source: the other sources' checkpoints do not move
    for b in range(0, total, block):
        whole[b:b + block] = (b // block) % n if b else n - 1
    return {"random": rng.integers(0, n, size=total).astype(np.uint8), "round robin": (np.arange(total) % n).astype(np.uint8), "whole blocks": whole}


def border_ranges(total, rng):
    block, narrow = msbwt.source_block_rows(), msbwt.source_narrow_rows()
    at = sorted({p for p in (0, 1, block - 1, block, block + 1, 2 * block - 1, 2 * block, total - 1, total) if 0 <= p <= total})
    pairs = [(l, h) for l, h in itertools.product(at, at) if l <= h]
    for l in at + [3, 15, 16, 17, block - narrow, block - 7]:  # the last width counted from the bytes themselves, and the first that is not
        pairs += [(l, l + w) for w in (narrow - 1, narrow, narrow + 1) if 0 <= l and l + w <= total]
    lo = rng.integers(0, total + 1, size=2000)
    hi = rng.integers(0, total + 1, size=2000)
    pairs += [(int(min(a, b)), int(max(a, b))) for a, b in zip(lo, hi)]
    short = rng.integers(0, total - 40, size=300)  # what a present k-mer looks like
    pairs += [(int(a), int(a + w)) for a, w in zip(short, rng.integers(0, 40, size=300))]
    pairs += [(0, total), (total, total), (0, 0)]
    return np.array([p[0] for p in pairs], dtype=U64), np.array([p[1] for p in pairs], dtype=U64)


@pytest.mark.parametrize("rows", ["R - 1", "R", "R + 1", "2 R + 1"])
def test_checkpoint_borders_against_bincount(rows):
    block = msbwt.source_block_rows()
    total = {"R - 1": block - 1, "R": block, "R + 1": block + 1, "2 R + 1": 2 * block + 1}[rows]
    assert msbwt.source_narrow_rows() + 8 < block
    _, rle = border_case(total)
    b = msbwt.RleBWT(device=0)
    b.load_vector(rle)
    assert b.get_total_size() == total
    rng = np.random.default_rng(total)
    l, h = border_ranges(total, rng)
    for n in (1, 2, 3, 8, 32):
        for name, sources in source_patterns(total, n, rng).items():
            b.set_sources(sources, n)
            assert b.source_count() == n
            want = np.stack([np.bincount(sources[int(a):int(z)], minlength=n) for a, z in zip(l, h)]).astype(U64)
            assert np.array_equal(b.source_totals(), np.bincount(sources, minlength=n).astype(U64)), (n, name)
            got = b.range_sources(l, h)
            assert got.shape == (l.size, n) and np.array_equal(got, want), (n, name, np.argwhere(got != want)[:5])
            assert np.array_equal(device_range_sources(b, l, h), want), (n, name)
            assert not got[l == h].any() and np.array_equal(got[(l == 0) & (h == total)][0], b.source_totals())


# ---- 2. the per-input identity, against the oracle ----

def cyclic_kmers(sets, k, rng, most=400):
    """k-mers cut from read + '$' + read of the collection's reads (as symbol codes): those across the '$' hold it."""
    out = []
    for reads in sets:
        for r in reads:
            text = r + "$" + r
            out += [text[i:i + k] for i in range(0, len(text) - k + 1)] if k else [""]
    out = sorted(set(out))
    if len(out) > most:
        out = [out[i] for i in rng.choice(len(out), size=most, replace=False)]
    codes = {c: i for i, c in enumerate("$ACGNT")}
    return np.array([[codes[c] for c in q] for q in out], dtype=np.uint8).reshape(len(out), k)


def oracle_columns(orc, rles, kmers):
    cols = []
    for r in rles:
        if len(r) == 0:
            cols.append(np.zeros(kmers.shape[0], dtype=U64))
        else:
            ref = orc.OracleRleBWT()
            ref.load_vector(r)
            cols.append(ref.count_kmers(kmers))
    return np.stack(cols, axis=1).astype(U64)


@pytest.mark.parametrize("n", [2, 3, 8, 32])
def test_every_column_is_the_count_in_that_input(orc, n):
    sets = ragged_collection(n, 0)
    assert [] in sets and [""] in sets
    rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
    merged = orc.OracleRleBWT()
    merged.load_vector(naive_rle(orc, sum(sets, [])))
    b = msbwt.RleBWT(device=0)
    b.load_merged_many(rles, keep_sources=True)
    assert b.source_count() == n
    assert b.source_totals().tolist() == [rle_total(r) for r in rles]
    rng = np.random.default_rng(n)
    seen_dollar = False
    for k in (0, 1, 5, 31):
        present = cyclic_kmers(sets, k, rng)
        if n > 2:
            assert present.shape[0] >= (1 if k == 0 else 5)
        absent = np.array([1, 2, 3, 5, 0, 4], dtype=np.uint8)[rng.integers(0, 6, size=(100 if k >= 5 else 0, k))]
        kmers = np.ascontiguousarray(np.concatenate([present, absent]))
        seen_dollar |= bool((present == 0).any())
        want = oracle_columns(orc, rles, kmers)
        assert np.array_equal(want.sum(axis=1, dtype=U64), merged.count_kmers(kmers))
        got = b.count_kmers_by_source(kmers)
        assert got.shape == (kmers.shape[0], n) and np.array_equal(got, want), (k, np.argwhere(got != want)[:5])
        assert np.array_equal(device_counts_by_source(b, kmers), want), k
        if k >= 5:
            assert (want[present.shape[0]:].sum(axis=1) == 0).any()  # absent ones among them
            bad = kmers.copy()
            row = kmers.shape[0] // 2
            bad[row, k // 2] = 6
            torch = _torch()
            out = device_counts_by_source(b, bad, check=False)
            with pytest.raises(MsbwtError) as err:
                b.device_status(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
            assert err.value.code == _lib.ERR_INVALID_SYMBOL
            assert (out[row] == ALL_ONES).all()
            keep = np.arange(kmers.shape[0]) != row
            assert np.array_equal(out[keep], want[keep])
            with pytest.raises(MsbwtError) as err:
                b.count_kmers_by_source(bad)
            assert err.value.code == _lib.ERR_INVALID_SYMBOL
    assert seen_dollar or n == 2


# ---- 3. knobs do not matter ----

def test_knobs_do_not_matter(orc):
    (flat, offsets), expected = read_set("plain_100")
    n = offsets.size - 1
    builder = msbwt.RleBWT(device=0)
    cuts = [0, n // 4, n // 4 + n // 3, n]
    rles = [builder.build_from_reads((flat, offsets[lo:hi + 1])) for lo, hi in zip(cuts[:-1], cuts[1:])]
    rng = np.random.default_rng(5)
    length = int(offsets[1])
    reads = flat.reshape(n, length)
    rows, starts = rng.integers(0, n, size=2000), rng.integers(0, length - 30, size=2000)
    derived = np.stack([reads[r, s:s + 31] for r, s in zip(rows, starts)])
    kmers = np.ascontiguousarray(np.concatenate([derived, np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=(500, 31))]]))
    want = oracle_columns(orc, rles, kmers)
    assert int(want[:2000].sum(axis=1).min()) >= 1 and (want > 0).sum(axis=0).min() > 100  # every part answers some

    b = msbwt.RleBWT(device=0)
    b.load_merged_many(rles, keep_sources=True)
    assert b.get_total_size() == rle_total(expected)
    assert np.array_equal(b.count_kmers_by_source(kmers), want)
    for setter, value in ((b.set_sparse_table, 0), (b.set_query_length, 31), (b.set_sparse_table, -1), (b.set_table_depth, 6)):
        setter(value)
        assert b.source_count() == 3
        assert np.array_equal(b.count_kmers_by_source(kmers), want), (setter.__name__, value)
        assert np.array_equal(device_counts_by_source(b, kmers), want), (setter.__name__, value)

    runs = msbwt.RleBWT(device=0)
    runs.set_block_format("runs")
    runs.load_merged_many(rles, keep_sources=True)
    assert runs.get_block_format() == "runs" or runs.get_block_format() == 1
    assert runs.source_count() == 3
    assert np.array_equal(runs.count_kmers_by_source(kmers), want)

    merged, sources = builder.merge_many(rles, return_sources=True)  # the vector through the host, onto an index loaded from the bytes
    assert np.array_equal(merged, expected)
    plain = msbwt.RleBWT(device=0)
    plain.load_vector(merged)
    assert plain.source_count() == 0
    plain.set_sources(sources)
    assert plain.source_count() == 3
    assert np.array_equal(plain.count_kmers_by_source(kmers), want)
    l, h = plain.kmer_ranges(kmers)
    assert np.array_equal(plain.range_sources(l, h), want)


def test_the_vector_travels_as_a_npy_beside_the_merged_file(orc, tmp_path):
    sets = ragged_collection(3, 2)
    rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
    paths = []
    for i, r in enumerate(rles):
        paths.append(str(tmp_path / ("in%d.npy" % i)))
        msbwt.bwt_converter.save_bwt_numpy(r, paths[-1])
    merged_path, sources_path = str(tmp_path / "merged.npy"), str(tmp_path / "merged.sources.npy")
    msbwt.bwt_util.merge_numpy_files(paths, merged_path, device=0, sources_out=sources_path)  # three files: "auto" takes the one pass for the vector's sake
    assert np.array_equal(np.load(merged_path), naive_rle(orc, sum(sets, [])))
    sources = np.load(sources_path)
    assert sources.dtype == np.uint8 and np.array_equal(sources, expected_sources(rles))
    with pytest.raises(ValueError):
        msbwt.bwt_util.merge_numpy_files(paths, merged_path, device=0, method="tree", sources_out=sources_path)
    later = msbwt.RleBWT(device=0)  # what a later process does
    later.load_numpy_file(merged_path)
    later.set_sources(np.load(sources_path), len(paths))
    kmers = cyclic_kmers(sets, 5, np.random.default_rng(1))
    assert np.array_equal(later.count_kmers_by_source(kmers), oracle_columns(orc, rles, kmers))


# ---- 4. wide ranges in closed form ----

def test_wide_ranges_in_closed_form(tmp_path):
    length = 3
    inputs = [{"A": 400000, "C": 400, "G": 12}, {"A": 300000, "C": 300, "G": 9, "T": 7}, {"A": 200000, "C": 200, "G": 6}]
    rles = [homopolymer_rle(counts, length, str(tmp_path / ("in%d.npy" % i))) for i, counts in enumerate(inputs)]
    b = msbwt.RleBWT(device=0)
    b.load_merged_many(rles, keep_sources=True)
    total = sum(sum(c.values()) for c in inputs) * (length + 1)
    assert b.get_total_size() == total > 3000 * msbwt.source_block_rows()
    stoi = msbwt.string_util.convert_stoi
    # a read c c c: `length` rotations start with c, length - 1 with c c, one with c $ and one with $
    cases = [("A", lambda c: c.get("A", 0) * length), ("AA", lambda c: c.get("A", 0) * (length - 1)), ("C", lambda c: c.get("C", 0) * length),
             ("$", lambda c: sum(c.values())), ("G$", lambda c: c.get("G", 0)), ("T", lambda c: c.get("T", 0) * length), ("TA", lambda c: 0)]
    for text, count in cases:
        got = b.count_kmers_by_source(stoi(text).reshape(1, -1))
        assert got.tolist() == [[count(c) for c in inputs]], text
    assert b.count_kmers_by_source(np.zeros((1, 0), dtype=np.uint8)).tolist() == [[sum(c.values()) * (length + 1) for c in inputs]]
    assert b.source_totals().tolist() == [sum(c.values()) * (length + 1) for c in inputs]


# ---- 5. beyond 2^32 rows ----

def test_beyond_2_to_32_rows(tmp_path):
    """4.41e9 merged rows from the three inputs of test_gpu_merge_many.py's case of the same name, merged, loaded and coloured in one
    call; ranges around row 2^32 and the k-mers A, T and $ against closed forms.  Measured on an MI355X: load_merged_many with the
    sources kept takes 0.80 s (the merge, the load and the attach of 4.41e9 rows) and the checks after it 0.02 s, so the read length
    stays at 29; where this test is the first of its process to start torch, that start-up adds about 13 s before the call."""
    started = time.perf_counter()
    torch = _torch()
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
    print("load_merged_many with sources, %d rows: %.2f s after %.2f s of set-up" % (total, time.perf_counter() - t0, t0 - started))
    assert b.get_total_size() == total and b.source_count() == 3
    assert b.source_totals().tolist() == totals
    assert b.device_bytes() > total

    # groups of equal rotations, in input order inside each: the '$' block has one group per letter, a letter's block `length` groups
    groups = []
    at = 0
    for c, repeat in [(c, 1) for c in "ACGNT"] + [(c, length) for c in "ACGNT"]:
        sizes = [counts.get(c, 0) for counts in inputs]
        for _ in range(repeat if sum(sizes) else 0):
            groups.append((at, sizes))
            at += sum(sizes)
    assert at == total

    def before(row):  # rows of every input in [0, row)
        out = [0] * len(inputs)
        for first, sizes in groups:
            for i, size in enumerate(sizes):
                out[i] += min(max(row - first, 0), size)
                first += size
        return out

    edge = 2 ** 32
    marks = [edge - 1, edge, edge + 1, edge - 1000, edge + 1000, edge - 10 ** 8, edge + 10 ** 8, 0, total]
    inside = [(first, sizes) for first, sizes in groups if first <= edge < first + sum(sizes)]
    assert len(inside) == 1
    first, sizes = inside[0]
    for size in sizes:  # the borders between the inputs of the group that holds row 2^32
        marks += [first - 1, first, first + 1]
        first += size
    marks = sorted({m for m in marks if 0 <= m <= total})
    pairs = [(l, h) for l, h in itertools.product(marks, marks) if l <= h]
    l, h = np.array([p[0] for p in pairs], dtype=U64), np.array([p[1] for p in pairs], dtype=U64)
    want = np.array([[z - a for a, z in zip(before(int(lo)), before(int(hi)))] for lo, hi in pairs], dtype=U64)
    assert any(int(lo) > edge for lo in l) and want.max() > 2 ** 31
    assert np.array_equal(b.range_sources(l, h), want)
    assert np.array_equal(device_range_sources(b, l, h), want)
    stoi = msbwt.string_util.convert_stoi
    for text, count in (("A", lambda c: c.get("A", 0) * length), ("T", lambda c: c.get("T", 0) * length), ("$", lambda c: sum(c.values()))):
        assert b.count_kmers_by_source(stoi(text).reshape(1, -1)).tolist() == [[count(c) for c in inputs]], text
    print("checks done %.2f s after the start" % (time.perf_counter() - started))


# ---- 6. lifetime ----

def _raw_set_sources(b, sources, n_rows, n_sources):
    import ctypes as C
    return _lib.lib().msbwt_rle_set_sources(b._h, None if sources is None else sources.ctypes.data_as(C.c_void_p), n_rows, n_sources)


def test_lifetime_of_the_attachment(orc):
    sets = ragged_collection(3, 1)
    rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
    merged = naive_rle(orc, sum(sets, []))
    sources = expected_sources(rles)
    total = sources.size
    kmers = cyclic_kmers(sets, 5, np.random.default_rng(0))
    want = oracle_columns(orc, rles, kmers)

    b = msbwt.RleBWT(device=0)
    assert _raw_set_sources(b, sources, total, 3) == _lib.ERR_NOT_LOADED
    b.load_vector(merged)
    bare = b.device_bytes()
    with pytest.raises(MsbwtError) as err:
        b.count_kmers_by_source(kmers[:, :5])
    assert err.value.code == _lib.ERR_NOT_LOADED and "no sources attached" in str(err.value)
    with pytest.raises(MsbwtError) as err:
        b.range_sources(np.zeros(1, dtype=U64), np.ones(1, dtype=U64))
    assert err.value.code == _lib.ERR_NOT_LOADED and "no sources attached" in str(err.value)

    b.set_sources(sources, 3)
    assert b.source_count() == 3 and np.array_equal(b.count_kmers_by_source(kmers), want)
    assert b.device_bytes() == bare + msbwt.source_index_plan(total, 3)
    b.set_sources(sources, 32)  # more sources than occur: the columns beyond stay zero
    assert b.device_bytes() == bare + msbwt.source_index_plan(total, 32)
    wide = b.count_kmers_by_source(kmers)
    assert np.array_equal(wide[:, :3], want) and not wide[:, 3:].any()
    b.set_sources(None)
    assert b.source_count() == 0 and b.device_bytes() == bare

    b.set_sources(sources)  # n_sources = the largest entry + 1
    assert b.source_count() == 3
    for wrong_rows, wrong_n in ((total - 1, 3), (total + 1, 3), (total, 0), (total, 33)):
        b.set_sources(sources, 3)
        assert _raw_set_sources(b, sources, wrong_rows, wrong_n) == _lib.ERR_INVALID_ARG, (wrong_rows, wrong_n)
        assert b.source_count() == 0
    b.set_sources(sources, 3)
    assert _raw_set_sources(b, sources, total, 2) == _lib.ERR_INVALID_ARG  # a byte >= n_sources, found on the device
    assert b.source_count() == 0 and b.device_bytes() == bare
    late = sources.copy()
    late[-1] = 3
    assert _raw_set_sources(b, late, total, 3) == _lib.ERR_INVALID_ARG
    assert b.source_count() == 0

    b.set_sources(sources, 3)
    twin = b.replicate(0)
    assert twin.source_count() == 3 and twin.source_totals().tolist() == b.source_totals().tolist()
    assert twin.device_bytes() == b.device_bytes()
    assert np.array_equal(twin.count_kmers_by_source(kmers), want)
    l, h = b.kmer_ranges(kmers)
    assert np.array_equal(twin.range_sources(l, h), b.range_sources(l, h))

    with pytest.raises(MsbwtError) as err:  # a range no search produces: all-ones and the consistency flag, never an address
        b.range_sources(np.array([5, 0], dtype=U64), np.array([4, total + 1], dtype=U64))
    assert err.value.code == _lib.ERR_INTERNAL
    assert np.array_equal(b.count_kmers_by_source(kmers), want)  # and the handle answers on

    b.load_vector(merged)  # any load drops the attachment
    assert b.source_count() == 0 and b.device_bytes() == bare
    with pytest.raises(MsbwtError) as err:
        b.count_kmers_by_source(kmers)
    assert err.value.code == _lib.ERR_NOT_LOADED
    b.load_merged_many(rles, keep_sources=True)
    assert b.source_count() == 3
    b.load_merged_many(rles)  # the plain form keeps no vector
    assert b.source_count() == 0
