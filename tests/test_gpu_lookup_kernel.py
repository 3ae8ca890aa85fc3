"""The bucket-lookup kernel (csrc/lookup_kernel.hip): batches whose k IS the depth of a complete sparse table.  Every count and the
device status must equal the CPU oracle's AND the same call served by the lanes kernel (set_search_kernel("lanes"), what
MSBWT_SEARCH=lanes selects); which kernel served a call is read from the label the launcher prints under MSBWT_VERBOSE.  The kernel
serves the shapes it was measured faster at -- query matrices, 40-bit tags (depths 30 and 31), a table fetched non-temporally (here:
forced, set_line_streaming) --, so the other depths of this file are checked to STAY with the lanes kernel and to count the same.
Needs an MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

from rust_msbwt_amd import RleBWT
from oracle import oracle as orc
from rle_random import random_kmers
import sparse_craft as sc
from test_gpu_sparse import ACGT, bwt_of, read_set

pytestmark = pytest.mark.gpu

DEPTHS = [16, 24, 25, 28, 30, 31]
SIZES = [1, 7, 8, 9, 63, 64, 65, 4097]
TILE = 64                      # the lookup kernel serves batches of at least one tile ...
LOOKUP_FROM = 30               # ... at the depths whose tags have 40 bits
MAXU = np.uint64(0xFFFFFFFFFFFFFFFF)
LABEL = "lookup kernel <"


class World:
    pass


def load(reads, depth, mp):
    mp.delenv("MSBWT_SEARCH", raising=False)
    mp.setenv("MSBWT_VERBOSE", "1")
    mp.setenv("MSBWT_SPARSE_TABLE", str(depth))
    mp.setenv("MSBWT_SPARSE_TIERS", "0")
    rle = bwt_of(reads)
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    b = RleBWT()
    b.load_vector(rle)
    assert b.get_sparse_table() == depth and not b.get_sparse_tiers() and b.get_pair_index() and b.get_search_kernel() == "auto"
    b.set_line_streaming(1)        # (automatic from 4 GiB of random-access arrays on: the regime the lookup kernel serves)
    return b, ref


def expected(ref, q):
    """the oracle's counts; u64::MAX for a row holding a code >= 6 (the reference asserts there), and whether there is such a row"""
    bad = (q >= 6).any(axis=1)
    exp = np.full(len(q), MAXU, dtype=np.uint64)
    if (~bad).any():
        exp[~bad] = ref.count_kmers(np.ascontiguousarray(q[~bad]))
    return exp, bool(bad.any())


def device_counts(b, q):
    """-> (counts, error code of device_status or 0) of one asynchronous device-pointer call"""
    import torch
    dev = torch.device("cuda:0")
    d_k = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_out = torch.full((len(q),), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    b.count_kmers_device(d_k.data_ptr(), q.shape[1], len(q), d_out.data_ptr(), stream)
    code = 0
    try:
        b.device_status(stream)
    except Exception as e:                # (MsbwtError: the status word said so)
        code = e.code
    return d_out.cpu().numpy().view(np.uint64), code


def both_kernels(w, q, capfd):
    """the call under the automatic choice and under "lanes": -> (counts, status, served by the lookup kernel?) of each"""
    out = []
    for mode in ("auto", "lanes"):
        w.b.set_search_kernel(mode)
        capfd.readouterr()
        got, code = device_counts(w.b, q)
        out.append((got, code, LABEL in capfd.readouterr().err))
    w.b.set_search_kernel("auto")
    return out


def check(w, q, capfd, looked_up=None):
    q = np.ascontiguousarray(q)
    exp, any_bad = expected(w.ref, q)
    (got, code, label), (lgot, lcode, llabel) = both_kernels(w, q, capfd)
    assert np.array_equal(got, exp) and np.array_equal(lgot, exp), np.flatnonzero(got != exp)[:10]
    assert (code != 0) == any_bad and code == lcode
    assert not llabel                                    # "lanes" keeps the lanes kernel
    assert label == (len(q) >= TILE and q.shape[1] >= LOOKUP_FROM if looked_up is None else looked_up)
    return got


def mixed_queries(reads, k, seed):
    """present k-mers, one-symbol mutants, random k-mers, rows with '$' / 'N', rows with invalid codes -- shuffled"""
    rng = np.random.default_rng(seed)
    windows = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1).reshape(-1, k)
    pick = lambda m: windows[rng.integers(0, len(windows), size=m)].copy()
    mut = pick(1300)
    mut[np.arange(len(mut)), rng.integers(0, k, size=len(mut))] = ACGT[rng.integers(0, 4, size=len(mut))]
    odd = pick(500)
    odd[np.arange(len(odd)), rng.integers(0, k, size=len(odd))] = rng.choice([0, 4], size=len(odd))
    for r in range(40):                                     # several of them in one row
        odd[r, rng.integers(0, k, size=3)] = 4
    bad = pick(60)
    bad[np.arange(len(bad)), rng.integers(0, k, size=len(bad))] = rng.choice([6, 7, 9, 255], size=len(bad))
    q = np.concatenate([pick(1400), mut, random_kmers(seed, 900, k), odd, bad])
    rng.shuffle(q)
    return np.ascontiguousarray(q)


@pytest.fixture(scope="module", params=DEPTHS, ids=lambda d: "depth%d" % d)
def toy(request):
    depth = request.param
    mp = pytest.MonkeyPatch()
    w = World()
    w.depth = depth
    reads = read_set(21 + depth, 5000, 900, 80, repeats=6, err=0.005)
    # homopolymer reads and copies of one read: suffixes 255 and more wide (their ranges live in the side array)
    homo = np.stack([np.full(80, c, dtype=np.uint8) for c in (1, 5)] * 150 + [reads[3]] * 260)
    w.reads = np.concatenate([reads, homo])
    w.b, w.ref = load(w.reads, depth, mp)
    assert w.b.sparse_table_info()["side_entries"] > 0
    w.q = mixed_queries(w.reads, depth, 1000 + depth)
    assert len(w.q) >= max(SIZES)
    yield w
    mp.undo()


@pytest.mark.parametrize("n", SIZES)
def test_counts_and_status_equal_the_oracle_and_the_lanes_kernel(toy, n, capfd):
    w = toy
    q = w.q[:n]
    got = check(w, q, capfd)
    if n == max(SIZES):
        kinds = (q >= 6).any(axis=1), ((q == 0) | (q == 4)).any(axis=1)
        assert kinds[0].sum() > 20 and kinds[1].sum() > 200 and (got[~kinds[0]] >= 255).any() and (got == 0).any()
    # rows without invalid codes: the host-pointer call (pinned pipeline) agrees too
    clean = np.ascontiguousarray(q[(q < 6).all(axis=1)])
    if len(clean):
        assert np.array_equal(w.b.count_kmers(clean), w.ref.count_kmers(clean))


def test_other_calls_keep_the_lanes_kernel(toy, capfd):
    """k beyond the table's depth, ranges, 2-bit queries and search counters are not the lookup kernel's"""
    import rust_msbwt_amd as msbwt
    w = toy
    k = w.depth + 1
    windows = np.lib.stride_tricks.sliding_window_view(w.reads[:200], k, axis=1).reshape(-1, k)
    check(w, windows[:300], capfd, looked_up=False)
    q = np.ascontiguousarray(w.q[(w.q < 6).all(axis=1)][:1000])
    exp = w.ref.count_kmers(q)
    capfd.readouterr()
    l, h = w.b.kmer_ranges(q)
    assert np.array_equal(h - l, exp)
    plain = np.ascontiguousarray(q[np.isin(q, ACGT).all(axis=1)])
    assert np.array_equal(w.b.count_kmers_packed(msbwt.rle_bwt.pack_2bit(plain), w.depth), w.ref.count_kmers(plain))
    w.b.set_search_counters(True)
    assert np.array_equal(w.b.count_kmers(q), exp)
    cnt = w.b.search_counters(0)
    w.b.set_search_counters(False)
    assert cnt["table_steps"] > 0
    assert LABEL not in capfd.readouterr().err
    assert np.array_equal(w.b.count_kmers(q), exp)
    assert (LABEL in capfd.readouterr().err) == (w.depth >= LOOKUP_FROM)    # the same batch without counters is the lookup kernel's again


def test_a_table_the_caches_hold_keeps_the_lanes_kernel(toy, capfd):
    """without non-temporal line fetches (the automatic choice on an index this small) every batch is the lanes kernel's"""
    w = toy
    w.b.set_line_streaming(-1)
    try:
        assert not w.b.get_line_streaming()
        check(w, w.q[:2000], capfd, looked_up=False)
    finally:
        w.b.set_line_streaming(1)


@pytest.mark.parametrize("strands", ["forward", "both"])
def test_read_windows_equal_the_oracle_and_the_lanes_kernel(toy, strands, capfd):
    """fused read windows at k = depth (they stay with the lanes kernel: the lookup kernel serves query matrices)"""
    capfd.readouterr()
    w = toy
    k, reads = w.depth, np.ascontiguousarray(w.reads[890:930])      # toy reads and homopolymers
    windows = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1).reshape(-1, k)
    exp_f = w.ref.count_kmers(np.ascontiguousarray(windows))
    exp_r = w.ref.count_kmers(np.array([orc.reverse_complement_i(x) for x in windows], dtype=np.uint8))
    for mode in ("auto", "lanes"):
        w.b.set_search_kernel(mode)
        fwd, rc = w.b.count_read_kmers(reads, k, ascii=False, forward=True, revcomp=strands == "both")
        assert np.array_equal(fwd.reshape(-1), exp_f), mode
        assert rc is None or np.array_equal(rc.reshape(-1), exp_r), mode
    w.b.set_search_kernel("auto")
    assert (exp_f >= 255).any() and LABEL not in capfd.readouterr().err


CRAFTED = [(config, kind) for config in ("complete16", "complete25", "complete30", "complete31") for kind in ("tags", "chains")]


@pytest.fixture(scope="module", params=CRAFTED, ids=lambda p: "-".join(p))
def crafted(request):
    config, kind = request.param
    mp = pytest.MonkeyPatch()
    w = World()
    w.plan = sc.tags_plan(config) if kind == "tags" else sc.chains_plan(config)
    w.kind, w.depth = kind, w.plan.depth
    mp.setenv("MSBWT_FILTER", "0")                       # absent crafted queries must reach the lookup under "lanes" too
    w.b, w.ref = load(w.plan.reads, w.plan.depth, mp)
    info = w.b.sparse_table_info()
    assert info["buckets"] == w.plan.nbuckets and info["probe"] == w.plan.probe
    yield w
    mp.undo()


def test_crafted_keys(crafted, capfd):
    """tag 0, key 0 and the all-T key, low tag words shared inside a bucket (40-bit tags), entries 255 and more wide; chains that end
    exactly `probe` buckets from home at the table's first bucket, mid-table and in its last line, absent keys behind them"""
    w = crafted
    rows, names = sc.query_rows(w.plan, seed=7)
    q = np.ascontiguousarray(rows[:, -w.depth:])
    got = check(w, q, capfd)
    n = len(w.plan.crafted)
    assert np.array_equal(got[:n], np.array([c.mult for c in w.plan.crafted], dtype=np.uint64))   # the second witness: as often as wished
    if w.kind == "chains":   # the last chain ends in the last line the table has
        assert w.b.sparse_table_info()["bytes"] // 128 - 1 == w.plan.nbuckets - 1 + w.plan.probe
    else:
        assert got.max() >= 255
    # every tile of a large batch: the rows many times over, and a ragged last tile
    big = np.ascontiguousarray(np.tile(q, (40, 1))[:-37])
    assert np.array_equal(check(w, big, capfd), np.tile(got, 40)[:-37])
