"""The two-tier sparse table's fallback (csrc/sparse_table.hpp, csrc/lanes_kernel.hpp) against the CPU oracle at every pairing of its
depth d with the direct table the filter sends queries to: packed 15 / 16 / 17, flat 16, none -- and the rule that pairs them
(csrc/sparse_policy.hpp, sparse_tier_fits_direct: the direct table, once packed, is shallower than a two-tier level).  Each case asserts
the configuration the loader chose BEFORE it counts anything, so that a configuration the kernel cannot serve is never launched.
Needs an MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import rust_msbwt_amd as msbwt
from rust_msbwt_amd import RleBWT, _lib
from oracle import oracle as orc
from rle_random import random_kmers
from test_gpu_sparse import ACGT, load_pair, read_set, synth_bwt

pytestmark = pytest.mark.gpu
MsbwtError = msbwt.rle_bwt.MsbwtError

A = 1
# the symbols that follow a poly-A stretch in the junction reads: with A C G T = 0 1 2 3 as the direct table's key digits (last symbol
# least significant), A^n C x y has a key below 30 -- the first line of a packed table, whose A^dd entry (the poly-A reads) is far more
# than 65 535 wide: an escape line
JUNCTIONS = ("CGT", "CAG", "CCA", "CTA", "CAT", "CGA")
CODE = {"A": 1, "C": 2, "G": 3, "T": 5}

# direct table -> (environment, depth once built, packed, needs the big HBM)
DIRECT = {
    "packed15": ({"MSBWT_TABLE_DEPTH": 13, "MSBWT_TABLE_PACKED": 1}, 15, True, False),
    "packed16": ({"MSBWT_TABLE_DEPTH": 14, "MSBWT_TABLE_PACKED": 1}, 16, True, False),   # ~18 GB
    "packed17": ({"MSBWT_TABLE_DEPTH": 15, "MSBWT_TABLE_PACKED": 1}, 17, True, True),    # ~73 GB
    "flat16": ({"MSBWT_TABLE_DEPTH": 16, "MSBWT_TABLE_PACKED": 0}, 16, False, True),     # 68 GB
    "none": ({"MSBWT_TABLE_DEPTH": 0}, 0, False, False),
}

_CACHE = {}


def high_copy_read_set():
    """Reads of a random genome with errors (counts 1 and > 1), plus high-copy sequence -- 2000 poly-A reads and 2500 (AC)^40 reads, so that
    A^dd occurs ~1.3e5 times and (AC)-repeat dd-mers ~4e4 times each: escape lines in every packed table up to depth 17 -- plus one read per
    JUNCTIONS entry, random | A^40 | xyz | random, whose k-mers ending at xyz occur exactly once and fall back to the escape line."""
    if "reads" not in _CACHE:
        rng = np.random.default_rng(7)
        genome = read_set(17, 5000, GENOME_READS, 80, repeats=6, err=0.01)
        poly = np.full((2000, 80), A, dtype=np.uint8)
        ac = np.tile(np.array([CODE["A"], CODE["C"]], dtype=np.uint8), (2500, 40))
        junction = []
        for xyz in JUNCTIONS:
            r = np.concatenate([ACGT[rng.integers(0, 4, size=20)], np.full(40, A, dtype=np.uint8),
                                np.array([CODE[c] for c in xyz], dtype=np.uint8), ACGT[rng.integers(0, 4, size=17)]])
            junction.append(r)
        reads = np.ascontiguousarray(np.concatenate([genome, poly, ac, np.stack(junction)]))
        _CACHE["reads"] = reads
        _CACHE["rle"] = synth_bwt(reads)
    return _CACHE["reads"], _CACHE["rle"]


def query_mix(reads, k, rng, genome_reads=None):
    """present (once-only among them), absent, one-symbol mutants and k-mers holding '$' / 'N' (present and mutants mostly from the first
    `genome_reads` reads: the genome's, where the errors are)"""
    windows = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1).reshape(-1, k)
    gw = windows[:(genome_reads or len(reads)) * (reads.shape[1] - k + 1)]
    present = np.concatenate([gw[rng.integers(0, len(gw), size=3000)], windows[rng.integers(0, len(windows), size=1000)]])
    mut = gw[rng.integers(0, len(gw), size=2000)].copy()
    mut[np.arange(len(mut)), rng.integers(0, k, size=len(mut))] = ACGT[rng.integers(0, 4, size=len(mut))]
    odd = windows[rng.integers(0, len(windows), size=600)].copy()
    odd[np.arange(len(odd)), rng.integers(0, k, size=len(odd))] = rng.choice([0, 4], size=len(odd))
    q = np.concatenate([present, random_kmers(k, 1500, k), mut, odd])
    rng.shuffle(q)
    return np.ascontiguousarray(q)


def junction_kmers(reads, k):
    """the k-mers of the junction reads that end at xyz (k <= 63): each occurs once, its last d symbols too"""
    return np.ascontiguousarray(reads[-len(JUNCTIONS):, 63 - k:63])


GENOME_READS = 1500


def counted(b, q):
    b.set_search_counters(True)
    got = b.count_kmers(q)
    cnt = b.search_counters(0)
    b.set_search_counters(False)
    return got, cnt


@pytest.mark.parametrize("direct", list(DIRECT))
@pytest.mark.parametrize("depth", [16, 17])
def test_two_tier_fallback_at_every_depth_pairing(depth, direct, monkeypatch):
    """Two-tier table of depth d in front of each direct table: counts of present, once-only, absent, mutated and '$' / 'N' k-mers equal the
    oracle's for k in {d, d+1, dd, dd+1, 31, 32, 33, 64}; a lookup that ends in the filter goes on through the direct table's line -- an
    escape line and its side entry for the junction k-mers.  Where the direct table would be as deep as d or deeper (packed 16 or 17 against
    d = 16, packed 17 against d = 17) the load fails with MSBWT_ERR_INVALID_ARG; the complete table of that depth then serves beside it.
    (d = dd was allowed once: a d-symbol query that ended in the filter then counted symbols beyond its own.)"""
    env, dd, packed, big = DIRECT[direct]
    if big:
        import torch
        if torch.cuda.mem_get_info(0)[0] < 120 * 10**9:
            pytest.skip("needs 120 GB of free HBM")
    reads, rle = high_copy_read_set()
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    if direct == "flat16" and depth == 16:
        # a sparse table serves the suffixes deeper than the flat table it is built from: an explicit depth that is not is an error
        with pytest.raises(MsbwtError) as err:
            load_pair(rle, monkeypatch, depth, MSBWT_SPARSE_TIERS=1, **env)
        assert err.value.code == _lib.ERR_INVALID_ARG and "must exceed the direct table" in str(err.value)
        return
    if dd >= depth:
        # both depths explicit and two-tier asked for: they conflict (the kernel would cut depth - dd symbols, a wrapped count, or -- at
        # dd = depth -- search on past the last symbol of a k = depth query) -> an error
        for k, v in dict(env, MSBWT_SEARCH="lanes", MSBWT_SPARSE_TABLE=depth, MSBWT_SPARSE_TIERS=1).items():
            monkeypatch.setenv(k, str(v))
        b = RleBWT()
        with pytest.raises(MsbwtError) as err:
            b.load_vector(rle)
        assert err.value.code == _lib.ERR_INVALID_ARG and "shallower than it" in str(err.value), str(err.value)
        b.set_sparse_tiers(0)   # the complete table of that depth has no such limit
        b.load_vector(rle)
        assert b.get_sparse_table() == depth and not b.get_sparse_tiers() and b.get_table_depth() == dd and b.get_table_packed() == packed
        tiers = False
    else:
        b, _ = load_pair(rle, monkeypatch, depth, MSBWT_SPARSE_TIERS=1, **env)
        assert b.get_sparse_table() == depth and b.get_sparse_tiers() and b.sparse_table_info()["two_tier"]
        assert b.get_table_depth() == dd and b.get_table_packed() == packed and b.get_table_depth() < b.get_sparse_table()
        tiers = True
    tinfo = b.table_info()
    if packed:
        assert tinfo["escape_lines"] > 0 and tinfo["side_bytes"] == tinfo["escape_lines"] * 512, tinfo
    rng = np.random.default_rng(depth * 100 + dd)
    ks = sorted({k for k in (depth, depth + 1, dd, dd + 1, 31, 32, 33, 64) if k >= depth})
    fallbacks = 0
    for k in ks:
        q = query_mix(reads, k, rng, GENOME_READS)
        if k <= 63:
            q = np.ascontiguousarray(np.concatenate([q, junction_kmers(reads, k)]))
        exp = ref.count_kmers(q)
        assert (exp == 0).sum() > 200 and (exp == 1).sum() > 200 and (exp > 1).sum() > 200, k
        got, cnt = counted(b, q)
        assert np.array_equal(got, exp), k
        fallbacks += cnt["tier_fallbacks"]
        assert tiers or cnt["tier_fallbacks"] == 0, cnt
        plain = q[np.isin(q, ACGT).all(axis=1)]
        assert np.array_equal(b.count_kmers_packed(msbwt.rle_bwt.pack_2bit(plain), k), ref.count_kmers(plain)), k
    assert not tiers or fallbacks > 0
    # the junction k-mers alone: each suffix of d symbols occurs once (filter), and its last dd symbols lie on the direct table's escape line
    k = 31
    jq = np.ascontiguousarray(np.concatenate([junction_kmers(reads, k)] * 20))   # (more than one small-batch launch holds)
    assert np.array_equal(ref.count_kmers(jq), np.ones(len(jq), dtype=np.uint64))
    got, cnt = counted(b, jq)
    assert np.array_equal(got, np.ones(len(jq), dtype=np.uint64))
    if tiers:
        assert cnt["tier_fallbacks"] == len(jq), cnt
        if packed:
            assert cnt["escape_queries"] >= len(jq), cnt
    # the fused read windows, both strands
    sample = np.ascontiguousarray(np.concatenate([reads[:150], reads[1500:1550], reads[-len(JUNCTIONS):]]))
    fwd, rc = b.count_read_kmers(sample, k, ascii=False, forward=True, revcomp=True)
    windows = np.lib.stride_tricks.sliding_window_view(sample, k, axis=1)
    assert np.array_equal(fwd, ref.count_kmers(windows.reshape(-1, k)).reshape(fwd.shape))
    rcq = np.array([orc.reverse_complement_i(w) for w in windows.reshape(-1, k)], dtype=np.uint8)
    assert np.array_equal(rc, ref.count_kmers(rcq).reshape(rc.shape))


def test_declared_k16_keeps_the_direct_table_within_the_two_tier_depth(monkeypatch):
    """k = 16 declared, two-tier asked for, direct depth automatic: the sparse table is 16 deep, and the loader does not keep the deep direct table
    (packed 16 on this index) beside it, as it does beside a complete table where HBM is plentiful -- the direct table stays shallower than
    the two-tier table."""
    import torch
    if torch.cuda.mem_get_info(0)[0] < 120 * 10**9:
        pytest.skip("needs 120 GB of free HBM")
    # 7e7 symbols: the automatic direct table would be packed 16 deep, and it fits HBM beside the sparse one
    reads = read_set(19, 3_000_000, 700_000, 100, repeats=10, err=0.004)
    rle = synth_bwt(reads)
    monkeypatch.setenv("MSBWT_SEARCH", "lanes")
    monkeypatch.setenv("MSBWT_SPARSE_TIERS", "1")
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    b = RleBWT()
    b.set_query_length(16)
    b.load_vector(rle)
    assert b.get_sparse_table() == 16 and b.get_sparse_tiers()
    assert 0 < b.get_table_depth() < 16, b.get_table_depth()
    rng = np.random.default_rng(16)
    for k in (16, 17, 31):
        q = query_mix(reads[:20000], k, rng)
        got, cnt = counted(b, q)
        assert np.array_equal(got, ref.count_kmers(q)), k
        assert cnt["tier_fallbacks"] > 0, cnt


def test_explicit_two_tier_request_that_conflicts_fails_through_the_setter(monkeypatch):
    """A loaded index with an explicit packed depth-17 direct table and the complete sparse table of depth 16: switching it to the two-tier form
    is refused with MSBWT_ERR_INVALID_ARG and the reason (nothing is dropped silently); the index keeps counting exactly, and the complete form
    comes back when asked for."""
    import torch
    if torch.cuda.mem_get_info(0)[0] < 120 * 10**9:
        pytest.skip("needs 120 GB of free HBM")
    reads, rle = high_copy_read_set()
    b, ref = load_pair(rle, monkeypatch, 16, MSBWT_SPARSE_TIERS=0, MSBWT_TABLE_DEPTH=15, MSBWT_TABLE_PACKED=1)
    assert b.get_sparse_table() == 16 and not b.get_sparse_tiers() and b.get_table_depth() == 17
    rc = _lib.lib().msbwt_rle_set_sparse_tiers(b._h, 1)
    assert rc == _lib.ERR_INVALID_ARG
    msg = _lib.lib().msbwt_rle_last_error(b._h).decode()
    assert "two-tier" in msg and "shallower than it" in msg and "17" in msg, msg
    assert not b.get_sparse_tiers()
    q = query_mix(reads, 31, np.random.default_rng(3))
    exp = ref.count_kmers(q)
    assert np.array_equal(b.count_kmers(q), exp)
    b.set_sparse_tiers(0)
    assert b.get_sparse_table() == 16 and not b.get_sparse_tiers() and b.get_table_depth() == 17
    assert np.array_equal(b.count_kmers(q), exp)


def test_two_tier_second_level(monkeypatch):
    """MSBWT_SPARSE_TIERS=1 with k undeclared: the second, shallower level (17-symbol suffixes) is of the two-tier form too, and says so
    (sparse_table_info()["second_tier"]); 17 <= k < d go through it and its fallback exactly, also once it is switched off, back on, and
    in a replica."""
    reads = read_set(61, 2_000_000, 400_000, 100, repeats=20, err=0.004)
    rle = synth_bwt(reads)
    b, ref = load_pair(rle, monkeypatch, "auto", MSBWT_TABLE_DEPTH=9, MSBWT_SPARSE_TIERS=1)
    info = b.sparse_table_info()
    assert info["depth"] >= 19 and info["two_tier"] and info["second_depth"] == 17 and info["second_tier"], info
    assert b.get_table_depth() <= 17
    rng = np.random.default_rng(17)
    qs, exp = {}, {}
    for k in range(17, info["depth"]):
        windows = np.lib.stride_tricks.sliding_window_view(reads[:3000], k, axis=1).reshape(-1, k)
        mut = windows[rng.integers(0, len(windows), size=3000)].copy()
        mut[np.arange(len(mut)), rng.integers(0, k, size=len(mut))] = ACGT[rng.integers(0, 4, size=len(mut))]
        qs[k] = np.ascontiguousarray(np.concatenate([windows[::5], random_kmers(k, 3000, k), mut]))
        exp[k] = ref.count_kmers(qs[k])
        assert (exp[k] == 0).sum() > 100 and (exp[k] == 1).sum() > 100 and (exp[k] > 1).sum() > 100, k
        got, cnt = counted(b, qs[k])
        assert np.array_equal(got, exp[k]), k
        assert cnt["tier_fallbacks"] > 0 and cnt["table_steps"] > 0, (k, cnt)
    b.set_sparse_second(0)
    assert b.sparse_table_info()["second_depth"] == 0 and not b.sparse_table_info()["second_tier"]
    for k, q in qs.items():
        assert np.array_equal(b.count_kmers(q), exp[k]), k
    b.set_sparse_second(-1)
    info2 = b.sparse_table_info()
    assert info2["second_depth"] == 17 and info2["second_tier"]
    for k, q in qs.items():
        assert np.array_equal(b.count_kmers(q), exp[k]), k
    twin = b.replicate(b.device_ordinal())
    assert twin.sparse_table_info()["second_tier"]
    for k, q in qs.items():
        assert np.array_equal(twin.count_kmers(q), exp[k]), k


@pytest.mark.parametrize("depth", [30, 31])
def test_tiers_1_at_depths_without_a_two_tier_form_gives_the_complete_table(depth, monkeypatch):
    """Depths 30 and 31 (40-bit tags) have no two-tier form: MSBWT_SPARSE_TIERS=1 leaves them complete, and the counts exact."""
    reads = read_set(131 + depth, 5000, 900, 80, repeats=6, err=0.01)
    rle = synth_bwt(reads)
    b, ref = load_pair(rle, monkeypatch, depth, MSBWT_SPARSE_TIERS=1)
    assert b.get_sparse_table() == depth and not b.get_sparse_tiers() and not b.sparse_table_info()["two_tier"]
    rng = np.random.default_rng(depth)
    for k in (depth, 31, 33, 64):
        if k < depth:
            continue
        q = query_mix(reads, k, rng)
        exp = ref.count_kmers(q)
        assert (exp == 0).sum() > 200 and (exp == 1).sum() > 200 and (exp > 1).sum() > 200, k
        got, cnt = counted(b, q)
        assert np.array_equal(got, exp), k
        assert cnt["tier_fallbacks"] == 0 and cnt["table_steps"] > 0, cnt
