"""GPU parity at the sizes of the BASELINE.json configs (not only on toy genomes): the HIP path
through the C ABI against the CPU oracle on large samples, plus whole-batch equality of the two
search kernels.  Needs an MI355X and a few minutes (the C4 index alone takes about a minute of
host time to build)."""
import os
import sys
import time

import numpy as np
import pytest

import rust_msbwt_amd as msbwt
from rust_msbwt_amd import RleBWT
from oracle import oracle as orc
from conftest import ROOT

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
# device_bytes() of the human-scale index in run blocks with its depth-23 sparse table, as the test prints it (70.25 GB); it wants a quarter more free
RUN_INDEX_BYTES = 70_250_000_000


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def _count_matrix(torch, dev, bwt, d_q):
    n, k = d_q.shape
    out = torch.empty(n, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    bwt.count_kmers_device(d_q.data_ptr(), k, n, out.data_ptr(), stream)
    bwt.device_status(stream)
    return out


def _revcomp(codes):
    comp = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)  # string_util.rs:12
    return np.ascontiguousarray(comp[codes[:, ::-1]])


def _oracle_ranges_and_extensions(ref, q, suffixes=()):
    """{k': (l, h, ext)} for k' = k and every suffix length in `suffixes`, by the oracle alone: its constrain_range, last symbol first
    (the range after t steps is the range of the last t symbols), empty ranges as (0, 0); ext[:, c] = the width of
    constrain_range(c, l, h), the count of c . row."""
    n, k = q.shape
    l = np.zeros(n, dtype=np.uint64)
    h = np.full(n, ref.get_total_size(), dtype=np.uint64)
    out = {}
    for t in range(k + 1):
        if t == k or t in suffixes:
            bounds = [ref.constrain_ranges(np.full(n, c, dtype=np.uint8), l, h) for c in range(6)]
            ext = np.stack([bh - bl for bl, bh in bounds], axis=1)
            el, eh = l.copy(), h.copy()
            el[l == h] = 0
            eh[l == h] = 0
            out[t] = (el, eh, ext)
        if t < k:
            l, h = ref.constrain_ranges(np.ascontiguousarray(q[:, k - 1 - t]), l, h)
    return out


def _check_ranges_and_extensions(bwt, q, expected, what):
    el, eh, eext = expected
    l, h = bwt.kmer_ranges(q)
    ext = bwt.count_kmer_extensions(q)
    assert np.array_equal(l, el) and np.array_equal(h, eh), what
    assert np.array_equal(ext, eext), what
    assert np.array_equal(bwt.count_kmers(q), eh - el) and np.array_equal(ext.sum(axis=1), eh - el), what


def test_c3_full_all_read_kmers_fused_both_strands():
    """BASELINE configs[2] at full size: ALL 31-mers of ALL 1 547 217 reads (1.857e8 windows), forward
    and reverse-complemented, prepared in-kernel; 1e6 sampled windows per strand against the oracle."""
    import synth
    torch, dev = _torch()
    npy, reads = synth.workload_index("c3")
    k = 31
    nread, rlen = reads.shape
    wins = rlen - k + 1
    bwt = RleBWT(device=0)
    bwt.load_numpy_file(npy)
    ref = orc.OracleRleBWT()
    ref.load_numpy_file(npy)
    assert bwt.get_total_size() == ref.get_total_size() == nread * (rlen + 1)
    d_reads = torch.from_numpy(reads).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = {}
    for mode in ("lanes", "groups"):
        bwt.set_search_kernel(mode)
        fwd = torch.empty(nread * wins, dtype=torch.int64, device=dev)
        rc = torch.empty(nread * wins, dtype=torch.int64, device=dev)
        bwt.count_read_kmers_device(d_reads.data_ptr(), rlen, nread, k, False, fwd.data_ptr(), rc.data_ptr(), stream)
        bwt.device_status(stream)
        outs[mode] = (fwd, rc)
    # the two search kernels agree on every one of the 3.7e8 counts
    assert torch.equal(outs["lanes"][0], outs["groups"][0]) and torch.equal(outs["lanes"][1], outs["groups"][1])
    fwd, rc = outs["lanes"]
    assert int(fwd.min()) >= 1  # every window occurs at least in its own read
    rng = np.random.default_rng(31)
    ids = np.sort(rng.choice(nread * wins, size=1_000_000, replace=False))
    windows = np.ascontiguousarray(reads[(ids // wins)[:, None], (ids % wins)[:, None] + np.arange(k)[None, :]])
    d_ids = torch.from_numpy(ids).to(dev)
    exp_f = ref.count_kmers(windows, nthreads=NCPU)
    exp_r = ref.count_kmers(_revcomp(windows), nthreads=NCPU)
    assert np.array_equal(fwd[d_ids].cpu().numpy().astype(np.uint64), exp_f)
    assert np.array_equal(rc[d_ids].cpu().numpy().astype(np.uint64), exp_r)
    # the explicit n x k matrix path gives the same counts for the sampled windows
    got_m = _count_matrix(torch, dev, bwt, torch.from_numpy(windows).to(dev))
    assert np.array_equal(got_m.cpu().numpy().astype(np.uint64), exp_f)


def test_c4_real_bwt_random_and_read_derived_31mers():
    """BASELINE configs[3]'s index and batch at full size on one GPU: the MSBWT of 12 888 833 reads
    (1.95e9 symbols, built here in the reference's ordering), 1e8 random 31-mers (1e6 sampled against
    the oracle, whole batch lanes == groups) and 2e7 read-derived 31-mers."""
    import synth
    torch, dev = _torch()
    npy, reads = synth.workload_index("c4")
    k = 31
    bwt = RleBWT(device=0)
    bwt.load_numpy_file(npy)
    ref = orc.OracleRleBWT()
    ref.load_numpy_file(npy)
    total = ref.get_total_size()
    assert bwt.get_total_size() == total == reads.shape[0] * (reads.shape[1] + 1)
    assert [bwt.get_symbol_count(s) for s in range(6)] == [ref.get_symbol_count(s) for s in range(6)]
    rng = np.random.default_rng(41)
    for name, q in (("random", synth.random_kmers(100_000_000, k, synth.CONFIGS["c4"]["qseed"])),
                    ("reads", synth.read_kmers(reads, k, limit=20_000_000, seed=7))):
        d_q = torch.from_numpy(q).to(dev)
        bwt.set_search_kernel("lanes")
        a = _count_matrix(torch, dev, bwt, d_q)
        bwt.set_search_kernel("groups")
        b = _count_matrix(torch, dev, bwt, d_q)
        assert torch.equal(a, b), name
        ids = np.sort(rng.choice(len(q), size=1_000_000, replace=False))
        exp = ref.count_kmers(q[ids], nthreads=NCPU)
        assert np.array_equal(a[torch.from_numpy(ids).to(dev)].cpu().numpy().astype(np.uint64), exp), name
        if name == "reads":
            assert int(a.min()) >= 1
        del d_q, a, b
    # Round 6: the TWO-TIER form of the sparse table on this read set (0.5 % substitutions: 2.4e8 distinct 23-mers, 3.7 x its genome's, most of
    # them error k-mers that occur once).  Solid, once-only and absent 31-mers -- read windows, and read windows with one symbol changed --
    # count n / 1 / 0 exactly as with the complete table and as the oracle says; the table holds entries only for the suffixes that occur
    # at least twice.
    bwt.set_search_kernel("lanes")
    q = synth.read_kmers(reads, k, limit=12_000_000, seed=9)
    mut = q[:4_000_000].copy()
    mut[np.arange(len(mut)), rng.integers(0, k, size=len(mut))] = np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=len(mut))]
    q = np.ascontiguousarray(np.concatenate([q, mut]))
    d_q = torch.from_numpy(q).to(dev)
    complete = _count_matrix(torch, dev, bwt, d_q)
    info0 = bwt.sparse_table_info()
    assert info0["depth"] == 23 and not info0["two_tier"]
    bwt.set_sparse_tiers(1)
    info1 = bwt.sparse_table_info()
    assert bwt.get_sparse_tiers() and info1["depth"] == 23 and info1["two_tier"]
    assert info1["entries"] + info1["filtered"] == info0["entries"] == info1["distinct"][23] and info1["filtered"] == info1["once"][23] > info1["entries"]
    bwt.set_search_counters(True)
    tiered = _count_matrix(torch, dev, bwt, d_q)
    cnt = bwt.search_counters(torch.cuda.current_stream(dev).cuda_stream)
    bwt.set_search_counters(False)
    assert torch.equal(tiered, complete)
    assert cnt["tier_fallbacks"] > 0.05 * len(q)      # the once-only suffixes (and a few false positives) took the direct table's path
    ids = np.sort(rng.choice(len(q), size=1_000_000, replace=False))
    exp = ref.count_kmers(q[ids], nthreads=NCPU)
    assert np.array_equal(tiered[torch.from_numpy(ids).to(dev)].cpu().numpy().astype(np.uint64), exp)
    assert (exp == 0).sum() > 50_000 and (exp == 1).sum() > 50_000 and (exp > 1).sum() > 500_000
    # k between the direct table's depth and the sparse table's, and beyond 32
    for kk in (17, 21, 22, 23, 24, 40):
        qs = np.ascontiguousarray(synth.read_kmers(reads, kk, limit=1_000_000, seed=kk))
        assert np.array_equal(_count_matrix(torch, dev, bwt, torch.from_numpy(qs).to(dev)).cpu().numpy().astype(np.uint64), ref.count_kmers(qs, nthreads=NCPU)), kk
    bwt.set_sparse_tiers(-1)
    assert not bwt.get_sparse_tiers() and torch.equal(_count_matrix(torch, dev, bwt, d_q), complete)


def test_stream_beyond_2_pow_33_symbols_hbm_regime():
    """A 9e9-symbol synthetic RLE stream (total > 2^33: positions and counts need more than 32 bits, the
    index is far larger than the Infinity Cache): present (LF-walk) and absent 31-mers and batched
    constrain_range at l, h > 2^32, all against the oracle on the same stream."""
    import synth
    sys.path.insert(0, ROOT)
    import bench
    torch, dev = _torch()
    rle, total = synth.rle_stream(9_000_000_000, 6.0, 123)
    assert total > 2**33
    bwt = RleBWT(device=0)
    bwt.load_vector(rle)
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    assert bwt.get_total_size() == total == ref.get_total_size()
    k = 31
    present = bench.walk_kmers(torch, np, bwt, dev, total, 2_000_000, k, 99)
    absent = bench.device_random_kmers(torch, dev, 0, 2_000_000, k, 98)
    d_q = torch.cat([present, absent])
    q = d_q.cpu().numpy()
    exp = ref.count_kmers(q, nthreads=NCPU)
    for mode in ("lanes", "groups"):
        bwt.set_search_kernel(mode)
        got = _count_matrix(torch, dev, bwt, d_q).cpu().numpy().astype(np.uint64)
        assert np.array_equal(got, exp), mode
    assert exp[:2_000_000].min() >= 1 and (exp[2_000_000:] == 0).mean() > 0.9
    # batched constrain_range with both bounds beyond 2^32
    rng = np.random.default_rng(17)
    n = 1_000_000
    a = rng.integers(2**32, total + 1, size=n, dtype=np.uint64)
    b = a + rng.integers(0, 5000, size=n).astype(np.uint64) * rng.integers(0, 2, size=n).astype(np.uint64)
    b = np.minimum(b, np.uint64(total))
    syms = rng.integers(0, 6, size=n).astype(np.uint8)
    gl, gh = bwt.constrain_ranges(syms, a, b)
    ol, oh = ref.constrain_ranges(syms, a, b)
    assert np.array_equal(gl, ol) and np.array_equal(gh, oh)
    assert int(gl.max()) > 2**32


def test_repeat_genome_read_set_built_on_the_gpu_and_counted():
    """bench.py --genome repeats in small: a 4e6-bp genome with the human repeat classes (synth.repeat_genome), 30x error-free reads,
    its exact MSBWT built by synth/bwt_reads.py msbwt_rle_repeats ON THE GPU -- the same bytes as the CPU build of the same tensors --
    loaded, and read-derived / walked / random k-mers counted against the oracle: high-copy k-mers (counts in the thousands), wide
    sparse-table entries in the side array, second lines at every step."""
    from synth import bwt_reads
    torch, dev = _torch()
    L = 150
    genome, cnt = bwt_reads.repeat_read_set(4_000_000, L, 30.0, 5)
    rle_cpu, totals, n_reads = bwt_reads.msbwt_rle_repeats(genome, cnt, L)
    rle, totals_gpu, n_gpu = bwt_reads.msbwt_rle_repeats(genome.to(dev), cnt.to(dev), L)
    assert n_gpu == n_reads and np.array_equal(totals, totals_gpu) and np.array_equal(rle, rle_cpu)
    total = int(totals.sum())
    bwt = RleBWT(device=0)
    bwt.load_vector(rle)
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    assert bwt.get_total_size() == ref.get_total_size() == total == n_reads * (L + 1)
    assert bwt.get_sparse_table() >= 19
    info = bwt.sparse_table_info()
    assert info["side_entries"] > 0          # suffixes of high-copy repeats: 255 or more wide
    sys.path.insert(0, ROOT)
    import bench
    for k in (23, 31, 59):
        walked = bench.walk_kmers(torch, np, bwt, dev, total, 300_000, k, 11 + k)      # drawn like read windows: repeats over-represented
        d_q = torch.cat([walked, bench.device_random_kmers(torch, dev, 0, 50_000, k, 3 + k)])
        exp = ref.count_kmers(d_q.cpu().numpy(), nthreads=NCPU)
        assert exp[:300_000].min() >= 1 and exp.max() > 1000
        for mode in ("lanes", "groups"):
            bwt.set_search_kernel(mode)
            got = _count_matrix(torch, dev, bwt, d_q).cpu().numpy().astype(np.uint64)
            assert np.array_equal(got, exp), (k, mode)
    bwt.set_search_kernel("auto")
    # a whole read as the query: as many occurrences as reads spell it
    reads = bwt_reads.reads_of(genome[:200_000 + L], cnt[:200_000], L)[:20_000]
    assert np.array_equal(bwt.count_kmers(reads), ref.count_kmers(reads, nthreads=NCPU))


def test_human_scale_9e10_symbols_against_the_oracle():
    """The size and the index the metric is quoted on: the exact MSBWT of 5.96e8 error-free reads, 9e10 symbols (positions
    beyond 2^36, 40-bit header counts with high bytes up to 20, the full index: sparse suffix table of depth 23 -- and, with it switched off, the 238 GB index of
    rounds 2-4 with its depth-17 packed table --, overlapping pair blocks addressed at human scale): 2e6 present (LF-walk) +
    2e6 random 31-mers under both search kernels, and 1e6 batched constrain_range calls with l, h > 2^36, all
    against the oracle on the same stream.  Then ranges and left-extension counts -- here every symbol's header counts have high bytes of
    their own -- of 2e5 of these 31-mers, their suffixes of 15 / 16 / 17 / 23 symbols and all ACGT k-mers of k = 1..6, under both kernels, with
    k undeclared and declared; MSBWT_ERR_OVERFLOW from the packed path's 32-bit counts for k = 1, 2; and the same 31-mers and 1e5 59-mers on
    the index in run blocks behind a sparse table (70.25 GB; loaded once the plane index is freed, skipped below 88 GB of free HBM).
    Needs ~250 GB of HBM and ~20 GB of host memory; 142 s on an MI355X, 22 s of them for the ranges, extensions and run blocks (this file:
    241 s before them, 250 s with them)."""
    import synth
    sys.path.insert(0, ROOT)
    import bench
    torch, dev = _torch()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 250 * 10**9:
        pytest.skip("needs 250 GB of free HBM")
    # bench.py's default index: the exact MSBWT of a 30x error-free read set, built on the GPU (synth/bwt_reads.py)
    from synth import bwt_reads
    genome, cnt = bwt_reads.read_set(int(bench.HUMAN_SYMBOLS * 150 / (30 * 151)), 150, 30.0, 77, device=dev)
    rle, totals, n_reads = bwt_reads.msbwt_rle(genome, cnt, 150)
    del genome, cnt
    torch.cuda.empty_cache()
    total = int(totals.sum())
    assert total == n_reads * 151 and abs(total - bench.HUMAN_SYMBOLS) < 1e-3 * bench.HUMAN_SYMBOLS and total > 2**36
    bwt = RleBWT(device=0)
    bwt.load_vector(rle)
    # the default index since round 5: sparse suffix table of depth 23 (3e9 distinct 23-mers, ~42 GB), a small direct table beside it
    assert bwt.get_total_size() == total and bwt.get_pair_index() and bwt.get_sparse_table() == 23 and bwt.get_table_depth() == 15
    assert bwt.get_line_streaming()   # 120 GB of pair blocks: their lines are fetched with the non-temporal hint
    info = bwt.sparse_table_info()
    assert 2.9e9 < info["entries"] < 3.1e9 and info["entries"] == info["distinct"][23] and info["bytes"] < 50e9, info
    # a real 30x BWT: present k-mers keep ranges ~ coverage wide, and the loader answers with overlapping pair blocks
    assert bwt.get_typical_range_width() >= 20 and bwt.get_pair_stride() == 96
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    assert ref.get_total_size() == total
    assert [bwt.get_symbol_count(s) for s in range(6)] == [ref.get_symbol_count(s) for s in range(6)]
    k = 31
    present = bench.walk_kmers(torch, np, bwt, dev, total, 2_000_000, k, 4242)
    absent = bench.device_random_kmers(torch, dev, 0, 2_000_000, k, 98)
    d_q = torch.cat([present, absent])
    q = d_q.cpu().numpy()
    exp = ref.count_kmers(q, nthreads=NCPU)
    assert exp[:2_000_000].min() >= 1
    for mode in ("lanes", "groups"):
        bwt.set_search_kernel(mode)
        got = _count_matrix(torch, dev, bwt, d_q).cpu().numpy().astype(np.uint64)
        assert np.array_equal(got, exp), mode
    # round 6: k between the direct table's depth and the sparse table's.  With k undeclared a SECOND sparse level (the 17-symbol suffixes,
    # 39 GB) serves 17 <= k < 23 -- the packed depth-17 direct table does not fit beside the first -- and k = 16 takes the direct table
    assert info["second_depth"] == 17 and 35e9 < info["second_bytes"] < 45e9 and bwt.device_bytes() < 260e9, info
    bwt.set_search_kernel("lanes")
    for kk in (16, 17, 19, 21, 22, 23, 24):
        short = torch.cat([present[:1_000_000, k - kk:], absent[:200_000, k - kk:]]).contiguous()
        got = _count_matrix(torch, dev, bwt, short).cpu().numpy().astype(np.uint64)
        assert np.array_equal(got, ref.count_kmers(short.cpu().numpy(), nthreads=NCPU)), kk
        assert got[:1_000_000].min() >= 1
    # the metric's own configuration (bench.py declares k = 31): the complete depth-31 table with 40-bit tags, more than 4e8 buckets;
    # a quarter of the present 31-mers have entries with l > 2^36
    t0 = time.time()
    bwt.set_query_length(31)
    info31 = bwt.sparse_table_info()
    assert bwt.get_sparse_table() == 31 and not bwt.get_sparse_tiers() and not info31["two_tier"] and info31["buckets"] > 4e8, info31
    got = _count_matrix(torch, dev, bwt, d_q).cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, exp)
    rng = np.random.default_rng(31)
    mut = present[:200_000].clone()
    mut[torch.arange(len(mut), device=dev), torch.from_numpy(rng.integers(0, k, size=len(mut))).to(dev)] = \
        torch.from_numpy(np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=len(mut))]).to(dev)
    got = _count_matrix(torch, dev, bwt, mut).cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, ref.count_kmers(mut.cpu().numpy(), nthreads=NCPU))
    sub = rng.choice(len(q), size=500_000, replace=False)
    packed_q = msbwt.rle_bwt.pack_2bit(np.ascontiguousarray(q[sub]))
    assert np.array_equal(bwt.count_kmers_packed(packed_q, k), exp[sub])
    long_q = bench.walk_kmers(torch, np, bwt, dev, total, 200_000, 59, 31)
    got = _count_matrix(torch, dev, bwt, long_q).cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, ref.count_kmers(long_q.cpu().numpy(), nthreads=NCPU)) and got.min() >= 1
    # two-tier asked for: depths 30 / 31 have no such form -- the declared k keeps the complete table
    bwt.set_sparse_tiers(1)
    assert bwt.get_sparse_table() == 31 and not bwt.get_sparse_tiers()
    # k undeclared, two-tier: depth 23 in front of the packed depth-15 direct table (the second level beside it, where it fits, is two-tier too)
    bwt.set_query_length(0)
    tinfo = bwt.sparse_table_info()
    assert bwt.get_sparse_table() == 23 and bwt.get_sparse_tiers() and bwt.get_table_depth() == 15 <= 23, tinfo
    assert tinfo["second_depth"] == 0 or tinfo["second_tier"], tinfo
    bwt.set_search_counters(True)
    got = _count_matrix(torch, dev, bwt, d_q).cpu().numpy().astype(np.uint64)
    bwt.set_search_counters(False)
    assert np.array_equal(got, exp)
    # back to the defaults
    bwt.set_sparse_tiers(-1)
    assert bwt.get_sparse_table() == 23 and not bwt.get_sparse_tiers() and bwt.get_table_depth() == 15
    assert bwt.sparse_table_info()["second_depth"] == 17
    print("k = 31 and two-tier checks at human scale: %.1f s" % (time.time() - t0))
    # without the sparse table the loader builds what rounds 2-4 measured: the depth-17 packed direct table (73 GB, 238 GB in all)
    bwt.set_sparse_table(0)
    assert bwt.get_sparse_table() == 0 and bwt.get_table_depth() == 17 and bwt.device_bytes() > 230e9
    bwt.set_search_kernel("lanes")
    got = _count_matrix(torch, dev, bwt, d_q).cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, exp)
    bwt.set_sparse_table(-1)
    assert bwt.get_sparse_table() == 23 and bwt.get_table_depth() == 15
    # k > 32 takes the other instantiation of the lanes kernel (6 words of symbols): 59-mers, fmlrc's long k
    bwt.set_search_kernel("auto")
    long_q = bench.walk_kmers(torch, np, bwt, dev, total, 500_000, 59, 7)
    got = _count_matrix(torch, dev, bwt, long_q).cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, ref.count_kmers(long_q.cpu().numpy(), nthreads=NCPU)) and got.min() >= 1
    # batched constrain_range with both bounds beyond 2^36
    rng = np.random.default_rng(23)
    n = 1_000_000
    a = rng.integers(2**36, total + 1, size=n, dtype=np.uint64)
    b = a + rng.integers(0, 5000, size=n).astype(np.uint64) * rng.integers(0, 2, size=n).astype(np.uint64)
    b = np.minimum(b, np.uint64(total))
    syms = rng.integers(0, 6, size=n).astype(np.uint8)
    gl, gh = bwt.constrain_ranges(syms, a, b)
    ol, oh = ref.constrain_ranges(syms, a, b)
    assert np.array_equal(gl, ol) and np.array_equal(gh, oh)
    assert int(gl.max()) > 2**36

    # ---- ranges and left-extension counts at this size.  Here every symbol's header counts have high bytes of their own (A 0..5, C 5..10,
    # G 10..15, T 15..20): two symbols' bytes mixed up, invisible at 6e9 symbols (tests/test_gpu_beyond_32_bits.py), give wrong bounds here.
    # 1e5 present + 1e5 absent 31-mers, their suffixes of 15 / 16 / 17 / 23 symbols, and all ACGT k-mers of k = 1..6
    t0 = time.time()
    q31 = np.ascontiguousarray(np.concatenate([q[:100_000], q[2_000_000:2_100_000]]))
    by_depth = _oracle_ranges_and_extensions(ref, q31, suffixes=(15, 16, 17, 23))
    sets = {kk: (np.ascontiguousarray(q31[:, k - kk:]), by_depth[kk]) for kk in (31, 15, 16, 17, 23)}
    acgt = np.array([1, 2, 3, 5], dtype=np.uint8)
    for kk in range(1, 7):
        every = np.ascontiguousarray(acgt[(np.arange(4 ** kk)[:, None] >> (2 * np.arange(kk - 1, -1, -1))[None, :]) & 3])
        sets[kk] = (every, _oracle_ranges_and_extensions(ref, every)[kk])
    l31 = by_depth[31][0][:100_000]
    assert np.array_equal(by_depth[31][1] - by_depth[31][0], exp[np.r_[0:100_000, 2_000_000:2_100_000]])
    beyond = float((l31 >= 2**36).mean())
    print("present 31-mers with l >= 2^36: %.1f %%; oracle ranges and extensions: %.1f s" % (100 * beyond, time.time() - t0))
    assert beyond >= 0.20, beyond
    for declared in (0, 31):
        bwt.set_query_length(declared)
        assert bwt.get_sparse_table() == (31 if declared else 23)
        for mode in ("lanes", "groups"):
            bwt.set_search_kernel(mode)
            for kk, (qs, expected) in sets.items():
                _check_ranges_and_extensions(bwt, qs, expected, (declared, mode, kk))
    # packed queries with 32-bit counts: a 1-mer or 2-mer occurs more than 2^32 times -- reported, not truncated
    for kk in (1, 2):
        words = msbwt.rle_bwt.pack_2bit(sets[kk][0])
        counts = sets[kk][1][1] - sets[kk][1][0]
        assert counts.min() >= 2**32 and np.array_equal(counts, ref.count_kmers(sets[kk][0], nthreads=NCPU))
        with pytest.raises(msbwt.rle_bwt.MsbwtError) as err:
            bwt.count_kmers_packed(words, kk, count_bits=32)
        assert err.value.code == msbwt._lib.ERR_OVERFLOW, str(err.value)
        assert np.array_equal(bwt.count_kmers_packed(words, kk), counts)
    got32 = bwt.count_kmers_packed(msbwt.rle_bwt.pack_2bit(sets[16][0]), 16, count_bits=32)
    assert got32.dtype == np.uint32 and np.array_equal(got32.astype(np.uint64), sets[16][1][1] - sets[16][1][0])
    print("ranges, extensions and packed counts at human scale: %.1f s" % (time.time() - t0))
    # ---- run blocks at this size (MSBWT_BLOCKS=runs: 40-bit header counts with every high byte in use, run blocks behind a sparse table):
    # the plane index goes first -- the two do not fit side by side
    t0 = time.time()
    long_q = np.ascontiguousarray(long_q[:100_000].cpu().numpy())
    exp59 = _oracle_ranges_and_extensions(ref, long_q)[59]
    handle, bwt._h = bwt._h, None   # freed now, whoever still refers to the object (pytest.raises keeps the frames of the call that raised)
    msbwt._lib.lib().msbwt_rle_free(handle)
    del bwt, d_q, present, absent, mut, err
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < RUN_INDEX_BYTES + RUN_INDEX_BYTES // 4:
        pytest.skip("the run-block part needs %.0f GB of free HBM" % (1.25 * RUN_INDEX_BYTES / 1e9))
    runs = RleBWT(device=0)
    runs.set_block_format("runs")
    runs.load_vector(rle)
    print("run blocks at human scale: device_bytes() = %.2f GB, sparse depth %d, loaded in %.1f s" % (runs.device_bytes() / 1e9, runs.get_sparse_table(), time.time() - t0))
    assert runs.get_block_format() == "runs" and runs.get_total_size() == total and not runs.get_pair_index()
    assert runs.get_sparse_table() >= 16
    for mode in ("lanes", "groups"):
        runs.set_search_kernel(mode)
        _check_ranges_and_extensions(runs, sets[31][0], sets[31][1], ("runs", mode, 31))
        _check_ranges_and_extensions(runs, long_q, exp59, ("runs", mode, 59))
    print("run blocks at human scale: %.1f s" % (time.time() - t0))
