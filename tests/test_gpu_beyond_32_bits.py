"""k-mer ranges, left-extension counts and both block formats on an index of more than 2^32 symbols, against the CPU oracle.

A count is h - l: the high bytes of two 40-bit bounds cancel, and where the sparse table's range is the answer the count kernels read
the entry's width and never its 40-bit `lo`.  So a wrong shift, a truncated `lo` or a 32-bit line index leaves every count right and
every range wrong -- and no index of a few hundred thousand symbols can tell.  This module builds the exact MSBWT of an error-free 30x
read set of 6e9 symbols on the GPU (synth/bwt_reads.py) once, computes every expected range, extension count and count from the oracle
alone (oracle/msbwt_oracle.c: constrain_range step by step, and count_kmers of the (k+1)-mers as a second route), asserts that the
queries really exercise what they are here for -- ranges beyond 2^32, ranges across a block border, and for every k = 1..8 the one
ACGT k-mer whose range STRADDLES 2^32, where the high bytes of l and h differ -- and then asks every index configuration that has a
range form.  Each configuration asserts what it loaded before it asks anything.

Memory: every test prints the device_bytes() of what it loads; HBM_GB holds the largest figure each test printed on a free 288 GB
MI355X, and a test is skipped when less than that plus a quarter (build scratch) is free.
Time on an MI355X: this file 56 s (21 s of it the fixtures: 4 s for the index, 15 s for the oracle's 2.9e7 constrain_range calls at
0.27 - 0.44 us each); `pytest -m gpu tests/test_gpu_config_sizes.py` took 241 s before the human-scale additions that came with this file and
250 s with them.  The human-scale test alone takes 120 s, so no query rows were cut.  Needs ~25 GB of host memory.  Run with `pytest -m gpu`."""
import time
import types

import numpy as np
import pytest

import rust_msbwt_amd as msbwt
from rust_msbwt_amd import RleBWT, _lib
from oracle import oracle as orc
from rle_random import random_kmers
from test_gpu_sparse import ACGT, oracle_ranges

pytestmark = pytest.mark.gpu

NCPU = 16
TWO32 = 1 << 32
SYMBOLS = 6_000_000_000
READ_LEN, COVERAGE, SEED = 150, 30.0, 2032
GENOME_SLICE = 200_000                       # the reads of these genome positions (~4e4) supply the read windows
KS = (12, 15, 16, 17, 22, 23, 24, 25, 27, 31, 32, 33, 59, 64, 65)
SHORT_KS = tuple(range(0, 9))                # k = 0, and ALL 4^k ACGT k-mers for k = 1..8
ROWS = {"windows": 25_000, "mutants": 12_000, "random": 9_000, "odd": 4_000}   # per k: 5e4 rows
# GB of device_bytes() each test printed in its first run (the replica test: two handles side by side); a test wants a quarter more free
HBM_GB = {"defaults": 88.60, "declared_k31": 88.60, "sparse27": 88.60, "sparse25": 87.60, "two_tier": 89.78, "no_sparse": 84.30,
          "no_pair": 7.30, "runs_sparse0": 2.82, "runs_sparseauto": 5.64, "host_planes": 88.60, "host_runs": 2.82, "replica": 2 * 88.60,
          "device_forms_planes": 88.60, "device_forms_runs": 5.64,
          "eight_digits_load": 34.36,   # (2^35 symbols: plane blocks 17.2 GB and the direct table; no pair index, no sparse table)
          "eight_digits_merge": 115.0,  # (no index: the one-pass merge of 2^35 rows by merge.hpp's plan_merge_many)
          "read_set": 6.49}     # (not an index: the peak of torch's allocations while the fixture builds the read set's BWT)


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def _gate(name):
    torch, dev = _torch()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 1.25e9 * HBM_GB[name]:
        pytest.skip("needs %.0f GB of free HBM" % (1.25 * HBM_GB[name]))


# ---- the index and what the oracle says about the queries -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def index():
    """(rle bytes, loaded oracle, total, a few reads) of the 6e9-symbol read set, built once"""
    from synth import bwt_reads
    torch, dev = _torch()
    _gate("read_set")
    t0 = time.time()
    genome, cnt = bwt_reads.read_set(int(SYMBOLS * READ_LEN / (COVERAGE * (READ_LEN + 1))), READ_LEN, COVERAGE, SEED, device=dev)
    reads = bwt_reads.reads_of(genome[:GENOME_SLICE + READ_LEN], cnt[:GENOME_SLICE], READ_LEN)
    rle, totals, n_reads = bwt_reads.msbwt_rle(genome, cnt, READ_LEN)
    del genome, cnt
    torch.cuda.empty_cache()
    total = int(totals.sum())
    assert total > TWO32 and total == n_reads * (READ_LEN + 1)
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    assert ref.get_total_size() == total
    print("index: %d symbols, %d reads, %d RLE bytes, %d sample reads; built and loaded into the oracle in %.1f s; peak of torch's allocations %.2f GB"
          % (total, n_reads, len(rle), len(reads), time.time() - t0, torch.cuda.max_memory_allocated(dev) / 1e9))
    return types.SimpleNamespace(rle=rle, ref=ref, total=total, reads=reads, n_reads=n_reads)


def query_mix(reads, k, rng):
    """test_gpu_tier_fallback.query_mix in larger numbers, and it says which rows are read windows: read windows, one-symbol mutants,
    random k-mers and windows holding one '$' / 'N'"""
    windows = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1).reshape(-1, k)
    win = windows[rng.integers(0, len(windows), size=ROWS["windows"])]
    mut = windows[rng.integers(0, len(windows), size=ROWS["mutants"])].copy()
    mut[np.arange(len(mut)), rng.integers(0, k, size=len(mut))] = ACGT[rng.integers(0, 4, size=len(mut))]
    odd = windows[rng.integers(0, len(windows), size=ROWS["odd"])].copy()
    odd[np.arange(len(odd)), rng.integers(0, k, size=len(odd))] = rng.choice([0, 4], size=len(odd))
    q = np.concatenate([win, mut, random_kmers(1000 + k, ROWS["random"], k), odd])
    is_window = np.zeros(len(q), dtype=bool)
    is_window[:len(win)] = True
    perm = rng.permutation(len(q))
    return np.ascontiguousarray(q[perm]), is_window[perm]


def all_kmers(k):
    """all 4^k ACGT k-mers (k = 0: three empty rows)"""
    if k == 0:
        return np.zeros((3, 0), dtype=np.uint8)
    digits = (np.arange(4 ** k)[:, None] >> (2 * np.arange(k - 1, -1, -1))[None, :]) & 3
    return np.ascontiguousarray(ACGT[digits])


def expect(ref, q, clock):
    """Everything a configuration is compared with, from the oracle alone: the range by constrain_range, last symbol first; the six
    extension bound pairs by constrain_range(c, l, h) on it; the count by count_kmers; and, for every eighth row, the extension counts
    again as count_kmers of the (k+1)-mers c . q."""
    n, k = q.shape
    t0 = time.time()
    if k:
        l, h = oracle_ranges(ref, q)
    else:
        l, h = np.zeros(n, dtype=np.uint64), np.full(n, ref.get_total_size(), dtype=np.uint64)
    bl = np.empty((n, 6), dtype=np.uint64)
    bh = np.empty((n, 6), dtype=np.uint64)
    for c in range(6):
        bl[:, c], bh[:, c] = ref.constrain_ranges(np.full(n, c, dtype=np.uint8), l, h)
    clock["constrain_calls"] += n * (k + 6)
    clock["constrain_s"] += time.time() - t0
    assert np.all(l <= h) and np.all(bl <= bh)
    ext = bh - bl
    cnt = ref.count_kmers(q, nthreads=NCPU)
    assert np.array_equal(h - l, cnt)                      # the oracle's two routes to a count agree
    sample = np.arange(0, n, 8)
    assert 10 * len(sample) >= n
    by_count = np.stack([ref.count_kmers(np.ascontiguousarray(np.hstack([np.full((len(sample), 1), c, dtype=np.uint8), q[sample]])),
                                         nthreads=NCPU) for c in range(6)], axis=1)
    assert np.array_equal(ext[sample], by_count), k        # ... and its two routes to the extension counts
    empty = l == h
    l[empty] = 0
    h[empty] = 0
    return types.SimpleNamespace(q=q, l=l, h=h, ext=ext, cnt=cnt, bl=bl, bh=bh)


@pytest.fixture(scope="module")
def cases(index):
    """k -> the query set and its expected answers, for KS (the mix) and SHORT_KS (exhaustive); the preconditions are asserted here, on
    the expected values, before the library is asked anything"""
    ref = index.ref
    rng = np.random.default_rng(SEED)
    clock = {"constrain_calls": 0, "constrain_s": 0.0}
    t0 = time.time()
    out = {}
    for k in KS:
        q, is_window = query_mix(index.reads, k, rng)
        c = out[k] = expect(ref, q, clock)
        present = c.cnt > 0
        window_present = is_window & present
        assert window_present.sum() == ROWS["windows"], k                    # error-free reads: every window occurs
        beyond = float((c.l[window_present] >= TWO32).mean())
        across = float(((c.l[present] >> np.uint64(8)) != (c.h[present] >> np.uint64(8))).mean())
        print("k = %d: %d rows, %d present; read windows with l >= 2^32: %.1f %%; present rows with l and h in different blocks: %.1f %%"
              % (k, len(q), int(present.sum()), 100 * beyond, 100 * across))
        assert beyond >= 0.20, (k, beyond)
        assert across >= 0.05, (k, across)
        assert (c.cnt == 0).sum() > 1000 and (c.cnt > 1).sum() >= ROWS["windows"] // 2, k
    straddling_bounds = 0
    for k in SHORT_KS:
        c = out[k] = expect(ref, all_kmers(k), clock)
        ranges = int(((c.l < TWO32) & (c.h >= TWO32)).sum())
        bounds = int(((c.bl < TWO32) & (c.bh >= TWO32) & (c.bl < c.bh)).sum())
        print("k = %d: %d rows; ranges with l < 2^32 <= h: %d; extension bound pairs that straddle 2^32: %d" % (k, len(c.q), ranges, bounds))
        if k:
            assert ranges >= 1, k                                            # (should 2^32 fall on a range edge: another SEED)
        straddling_bounds += bounds
    assert straddling_bounds >= 1
    print("expected values: %.1f s in all; oracle constrain_range: %d calls in %.1f s (%.2f us each)"
          % (time.time() - t0, clock["constrain_calls"], clock["constrain_s"], 1e6 * clock["constrain_s"] / clock["constrain_calls"]))
    return out


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def differences(got, exp, what):
    """[] when the arrays are equal, else one line that says how they differ"""
    got, exp = np.asarray(got).astype(np.uint64), np.asarray(exp).astype(np.uint64)
    if got.shape != exp.shape:
        return ["%s: shape %s, expected %s" % (what, got.shape, exp.shape)]
    if np.array_equal(got, exp):
        return []
    bad = np.argwhere(got != exp)
    first = tuple(bad[0])
    return ["%s: %d of %d values differ; first at %s: got %d (%#x), expected %d (%#x)"
            % (what, len(bad), got.size, first, int(got[first]), int(got[first]), int(exp[first]), int(exp[first]))]


def same(got, exp, what):
    found = differences(got, exp, what + " against the oracle")
    assert not found, found[0]


def check(b, c, what):
    """counts, ranges and extension counts of one query set: equal to the oracle's, and consistent among themselves -> what is not"""
    what = "%s, k = %d" % (what, c.q.shape[1])
    cnt = b.count_kmers(c.q)
    l, h = b.kmer_ranges(c.q)
    ext = b.count_kmer_extensions(c.q)
    found = (differences(cnt, c.cnt, what + ": count_kmers against the oracle") + differences(l, c.l, what + ": kmer_ranges l against the oracle")
             + differences(h, c.h, what + ": kmer_ranges h against the oracle")
             + differences(ext, c.ext, what + ": count_kmer_extensions against the oracle")
             + differences(h - l, cnt, what + ": h - l against the library's count")
             + differences(ext.sum(axis=1), cnt, what + ": sum of the six extension counts against the library's count"))
    if not np.all((cnt > 0) | ((l == 0) & (h == 0))):
        found.append(what + ": an empty range is not (0, 0)")
    return found


def check_all(b, cases, what, ks=KS + SHORT_KS):
    """every query set of `ks`; all that differs is reported at once"""
    found = []
    for k in ks:
        found += check(b, cases[k], what)
    assert not found, "%d checks failed:\n" % len(found) + "\n".join(found)


@pytest.fixture
def handles():
    """the handles a test loads: released when it ends, however it ends, so that the next load finds the HBM free"""
    made = []
    yield made
    for b in made:
        release(b)


def release(b):
    h, b._h = b._h, None
    if h:
        _lib.lib().msbwt_rle_free(h)
    _torch()[0].cuda.empty_cache()


def load(name, index, monkeypatch, handles, env=None, prepare=None):
    """a handle on the index under `env`, after `prepare`; `name`: the test's entry in HBM_GB"""
    _gate(name)
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, str(v))
    b = RleBWT(device=0)
    handles.append(b)
    if prepare:
        prepare(b)
    t0 = time.time()
    b.load_vector(index.rle)
    assert b.get_total_size() == index.total
    print("%s: loaded in %.1f s, device_bytes() = %.2f GB, sparse depth %d, direct depth %d, %s blocks"
          % (env or "defaults", time.time() - t0, b.device_bytes() / 1e9, b.get_sparse_table(), b.get_table_depth(), b.get_block_format()))
    return b


# ---- configurations ------------------------------------------------------------------------------------------------------------------
def test_defaults_auto_lanes_groups(index, cases, monkeypatch, handles):
    """k undeclared: the depth-23 sparse table with a second level or a deep direct table beside it, under each search kernel.
    device_bytes() 88.60 GB."""
    b = load("defaults", index, monkeypatch, handles)
    info = b.sparse_table_info()
    assert b.get_block_format() == "planes" and b.get_pair_index() and b.get_query_length() == 0
    assert b.get_sparse_table() == 23 and not b.get_sparse_tiers() and (info["second_depth"] == 17 or b.get_table_depth() >= 16), info
    for mode in ("auto", "lanes", "groups"):
        b.set_search_kernel(mode)
        assert b.get_search_kernel() == mode
        if mode != "auto":
            assert b.search_kernel_for(31) == mode
        check_all(b, cases, "defaults, " + mode)


def test_declared_k31_answers_from_the_entry(index, cases, monkeypatch, handles):
    """set_query_length(31): the depth-31 table with 40-bit tags; a 31-mer's range is its entry's (lo, lo + width).
    device_bytes() 88.60 GB."""
    b = load("declared_k31", index, monkeypatch, handles, prepare=lambda b: b.set_query_length(31))
    assert b.get_query_length() == 31 and b.get_sparse_table() == 31 and not b.get_sparse_tiers() and b.get_pair_index()
    check_all(b, cases, "declared k = 31")


@pytest.mark.parametrize("depth", [27, 25])
def test_sparse_table_with_32_bit_tags(depth, index, cases, monkeypatch, handles):
    """MSBWT_SPARSE_TABLE=27 / 25: the 12-slot layout; k equal to the depth is answered from the entry.
    device_bytes() 88.60 / 87.60 GB."""
    b = load("sparse%d" % depth, index, monkeypatch, handles, {"MSBWT_SPARSE_TABLE": depth})
    assert b.get_sparse_table() == depth and not b.get_sparse_tiers() and b.get_pair_index()
    check_all(b, cases, "sparse depth %d" % depth)


def test_two_tier_depth_23_through_the_direct_table(index, cases, monkeypatch, handles):
    """set_sparse_tiers(1): entries for the suffixes that occur at least twice in front of the packed depth-17 direct table; a hit cuts
    the 6 symbols between the two depths.  (Error-free 30x reads have next to no suffix that occurs once -- two of 1.99e8 here: the filter is all but empty,
    and the fallback through it is what tests/test_gpu_tier_fallback.py and the C4 test exercise.)  device_bytes() 89.78 GB."""
    b = load("two_tier", index, monkeypatch, handles, prepare=lambda b: b.set_sparse_tiers(1))
    info = b.sparse_table_info()
    assert b.get_sparse_table() == 23 and b.get_sparse_tiers() and info["two_tier"] and 0 < b.get_table_depth() < 23, info
    print("two-tier: %d entries, %d suffixes that occur once in the filter" % (info["entries"], info["filtered"]))
    assert info["entries"] + info["filtered"] == info["distinct"][23]
    check_all(b, cases, "two-tier depth 23")


def test_no_sparse_table_packed_direct_depth_17(index, cases, monkeypatch, handles):
    """MSBWT_SPARSE_TABLE=0: the packed depth-17 direct table answers k = 17 by itself.  device_bytes() 84.30 GB."""
    b = load("no_sparse", index, monkeypatch, handles, {"MSBWT_SPARSE_TABLE": 0})
    assert b.get_sparse_table() == 0 and b.get_table_depth() == 17 and b.get_table_packed() and b.get_pair_index()
    for mode in ("lanes", "groups"):
        b.set_search_kernel(mode)
        assert b.search_kernel_for(17) == mode
        check_all(b, cases, "no sparse table, " + mode)


def test_single_symbol_steps(index, cases, monkeypatch, handles):
    """set_pair_index(0): one symbol per step on the plane blocks alone.  device_bytes() 7.30 GB."""
    b = load("no_pair", index, monkeypatch, handles, prepare=lambda b: b.set_pair_index(0))
    assert not b.get_pair_index() and b.get_block_format() == "planes"
    for mode in ("lanes", "groups"):
        b.set_search_kernel(mode)
        assert b.search_kernel_for(31) == mode
        check_all(b, cases, "no pair index, " + mode)


@pytest.mark.parametrize("sparse", [0, "auto"])
def test_run_blocks(sparse, index, cases, monkeypatch, handles):
    """MSBWT_BLOCKS=runs: 40-bit header counts (hi03 / hi45 beside the overflow flag), the per-lane decode, extend.hip's other branch.
    device_bytes() 2.82 GB without a sparse table, 5.64 GB with the automatic one."""
    b = load("runs_sparse%s" % sparse, index, monkeypatch, handles, {"MSBWT_BLOCKS": "runs", "MSBWT_SPARSE_TABLE": sparse})
    assert b.get_block_format() == "runs" and not b.get_pair_index()
    assert (b.get_sparse_table() == 0) if sparse == 0 else (b.get_sparse_table() >= 16)
    for mode in ("lanes", "groups"):
        b.set_search_kernel(mode)
        check_all(b, cases, "run blocks, sparse %s, %s" % (sparse, mode))


@pytest.mark.parametrize("blocks", ["planes", "runs"])
def test_host_built_headers(blocks, index, cases, monkeypatch, handles):
    """MSBWT_BUILD=host: the block headers the host builders write, in both formats.  device_bytes() 88.60 / 2.82 GB."""
    b = load("host_" + blocks, index, monkeypatch, handles, {"MSBWT_BUILD": "host", "MSBWT_BLOCKS": blocks})
    assert b.get_block_format() == blocks
    check_all(b, cases, "host build, " + blocks, (31,) + SHORT_KS)


def test_replica_of_the_default_handle(index, cases, monkeypatch, handles):
    """msbwt_rle_replicate copies every array by its byte count: the copy answers alone.  device_bytes() 88.60 GB each, two side by side."""
    b = load("replica", index, monkeypatch, handles)
    twin = b.replicate(b.device_ordinal())
    handles.append(twin)
    print("default handle and its replica: device_bytes() = %.2f GB each" % (b.device_bytes() / 1e9))
    assert twin.device_bytes() == b.device_bytes() and twin.get_total_size() == index.total
    assert twin.get_sparse_table() == b.get_sparse_table() and twin.get_table_depth() == b.get_table_depth()
    release(b)                                                # the copy stands alone
    check_all(twin, cases, "replica", (24, 31))


# ---- once each on the default and on the run-block handle: device forms, fused reads, packed queries -------------------------------------
def _revcomp(codes):
    comp = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)
    return np.ascontiguousarray(comp[codes[:, ::-1]])


@pytest.mark.parametrize("blocks", ["planes", "runs"])
def test_device_forms_fused_reads_and_packed_queries(blocks, index, cases, monkeypatch, handles):
    """Device forms on an aligned and on an unaligned query buffer with a guard element behind each output, the fused read path on both
    strands, packed queries with 64- and 32-bit counts.  device_bytes() 88.60 GB (planes) / 5.64 GB (runs)."""
    torch, dev = _torch()
    b = load("device_forms_" + blocks, index, monkeypatch, handles, {"MSBWT_BLOCKS": blocks})
    assert b.get_block_format() == blocks
    ref = index.ref
    stream = torch.cuda.current_stream(dev).cuda_stream
    GUARD = 0x5A5A5A5A5A5A5A5A
    for k in (5, 31, 65):
        c = cases[k]
        n = len(c.q)
        for offset in (0, 1):                              # 16-byte aligned, and one byte off
            raw = torch.zeros(n * k + 16, dtype=torch.uint8, device=dev)
            raw[offset:offset + n * k] = torch.from_numpy(c.q.reshape(-1)).to(dev)
            d_l = torch.full((n + 1,), GUARD, dtype=torch.int64, device=dev)
            d_h = torch.full((n + 1,), GUARD, dtype=torch.int64, device=dev)
            d_e = torch.full((n * 6 + 1,), GUARD, dtype=torch.int64, device=dev)
            b.kmer_ranges_device(raw.data_ptr() + offset, k, n, d_l.data_ptr(), d_h.data_ptr(), stream)
            b.count_kmer_extensions_device(raw.data_ptr() + offset, k, n, d_e.data_ptr(), stream)
            b.device_status(stream)
            what = "%s, device form, k = %d, offset %d" % (blocks, k, offset)
            same(d_l[:n].cpu().numpy(), c.l, what + ": l")
            same(d_h[:n].cpu().numpy(), c.h, what + ": h")
            same(d_e[:n * 6].cpu().numpy().reshape(n, 6), c.ext, what + ": extensions")
            assert int(d_l[n]) == GUARD and int(d_h[n]) == GUARD and int(d_e[n * 6]) == GUARD, what
    # the fused read path, both strands
    sample = np.ascontiguousarray(index.reads[:2000])
    for k in (31, 47):
        fwd, rc = b.count_read_kmers(sample, k, ascii=False, forward=True, revcomp=True)
        windows = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(sample, k, axis=1).reshape(-1, k))
        exp_f = ref.count_kmers(windows, nthreads=NCPU)
        same(fwd.reshape(-1), exp_f, "%s, fused reads, k = %d, forward" % (blocks, k))
        same(rc.reshape(-1), ref.count_kmers(_revcomp(windows), nthreads=NCPU), "%s, fused reads, k = %d, reverse complement" % (blocks, k))
        assert exp_f.min() >= 1
    # packed queries, 64- and 32-bit counts
    c = cases[31]
    plain = np.isin(c.q, ACGT).all(axis=1)
    words = msbwt.rle_bwt.pack_2bit(np.ascontiguousarray(c.q[plain]))
    assert plain.sum() > 40_000
    got64 = b.count_kmers_packed(words, 31)
    got32 = b.count_kmers_packed(words, 31, count_bits=32)
    assert got64.dtype == np.uint64 and got32.dtype == np.uint32
    same(got64, c.cnt[plain], blocks + ", packed, 64-bit counts")
    same(got32, c.cnt[plain], blocks + ", packed, 32-bit counts")


# ---- the largest weight an RLE byte can have --------------------------------------------------------------------------------------------
def test_a_run_of_eight_digits_across_a_thread_border_loads(monkeypatch, handles):
    """The eighth digit of a run weighs 32^7 = 2^35 symbols, so no small stream has one.  Here the run's eight bytes lie at bytes
    13..20 of the stream, on both sides of byte 16, where the device walk (csrc/rle_subruns.hpp: 16 bytes to a thread) hands the
    count of a run's bytes from one thread to the next; the first seven digits are zero.  The loader's plane blocks equal the
    host builder's word for word (17.2 GB each)."""
    from rle_random import EIGHT_DIGITS
    from test_gpu_parity import _download_blocks, _host_blocks
    _gate("eight_digits_load")
    stream, total = EIGHT_DIGITS(), 13 + 2 ** 35 + 40
    monkeypatch.setenv("MSBWT_SPARSE_TABLE", "0")
    b = RleBWT(device=0)
    handles.append(b)
    b.set_pair_index(0)
    t0 = time.time()
    b.load_vector(stream)
    assert b.get_total_size() == total and b.get_block_format() == "planes"
    t1 = time.time()
    print("eight digits: device_bytes() = %.2f GB" % (b.device_bytes() / 1e9))
    dev = _download_blocks(b)
    release(b)
    host = _host_blocks(stream)
    t2 = time.time()
    assert dev.shape == host.shape == (total // 256 + 1, 8, 4)
    assert np.array_equal(dev, host)
    print("eight digits: load %.1f s, download and host build %.1f s, compare %.1f s" % (t1 - t0, t2 - t1, time.time() - t2))


def test_a_run_of_eight_digits_across_a_thread_border_merges(handles):
    """The same stream through the decoder of both merges: merged with nothing it comes back in canonical form -- expected from
    the runs alone (rle_random.canonical_runs, which tests/test_gpu_merge.py's small streams tie to the oracle's decoder): what
    the oracle would decode to does not fit a test."""
    from rle_random import EIGHT_DIGITS, canonical_runs
    _gate("eight_digits_merge")
    stream, empty, total = EIGHT_DIGITS(), np.empty(0, dtype=np.uint8), 13 + 2 ** 35 + 40
    want = canonical_runs(stream)
    assert want.size == stream.size and msbwt.rle_bwt.rle_total(want) == total
    t0 = time.time()
    m = RleBWT(device=0)
    handles.append(m)
    assert np.array_equal(m.merge(stream, empty), want)
    assert np.array_equal(m.merge(empty, stream), want)
    assert np.array_equal(m.merge_many([stream]), want)
    print("eight digits: three merges %.1f s" % (time.time() - t0))
