"""Read overlaps on the device (include/msbwt_hip.h, "read overlaps": msbwt_rle_read_overlaps[_device]) against tests/overlap_oracle.py,
which knows the BWT string alone, word for word on every output: ragged read sets against the oracle and, through overlap_edges,
against an all-against-all string comparison; steps with both bounds in one block and in two; random RLE streams that are no BWT;
every index form; batch shapes, pieces and odd addresses; the capacity contract; bad symbols; the guards in their order; the empty
batch and the empty index; ranges and records past 2^32 against the closed form over a run list; and the round trip from
extract_reads."""
import ctypes as C
import importlib

import numpy as np
import pytest

import overlap_oracle as O
from rle_random import random_stream, runs_to_bytes
from test_gpu_kmer_graph import FORMS
from test_gpu_spectrum import loaded
from test_overlap_oracle import CODE, LETTER, codes_of, overlap_read_set

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
SENTINEL = 77
TAIL = 8  # sentinel words behind a column's capacity
PER_QUERY = ("offsets", "matched", "edges", "stops")
COLUMNS = ("lengths", "first", "counts")
ALL_FORMS = dict(FORMS, **{"no sparse table": dict(sparse_table=0), "no direct table": dict(table_depth=0)})


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ragged(queries):
    """a list of code arrays -> (flat, offsets)"""
    return msbwt.rle_bwt.pack_reads([np.asarray(q, dtype=np.uint8) for q in queries])


def raw(b, queries, m, M=0, strand=0, capacity=None, device=False, want=PER_QUERY, total=True):
    """msbwt_rle_read_overlaps[_device] itself -> (return code, {name: array, or None where `want` leaves it out}, R).  queries: a list of
    code arrays or a (flat, offsets) pair.  capacity None: a counting call; else the columns hold capacity + TAIL sentinel words."""
    flat, offsets = queries if isinstance(queries, tuple) else ragged(queries)
    n = len(offsets) - 1
    out = {"offsets": np.full(n + 1, SENTINEL, dtype=U64), "matched": np.full(n, SENTINEL, dtype=U64), "edges": np.full(n, SENTINEL, dtype=U64),
           "stops": np.full(n, SENTINEL, dtype=np.uint8)}
    out = {k: (v if k in want else None) for k, v in out.items()}
    for name in COLUMNS:
        out[name] = None if capacity is None else np.full(capacity + TAIL, SENTINEL, dtype=U64)
    R = C.c_uint64(99)
    where_total = C.byref(R) if total else None
    if not device:
        rc = _lib.lib().msbwt_rle_read_overlaps(b._h, _ptr(flat), _ptr(offsets), n, m, M, strand, _ptr(out["offsets"]), *[_ptr(out[c]) for c in COLUMNS], capacity or 0,
                                                where_total, _ptr(out["matched"]), _ptr(out["edges"]), _ptr(out["stops"]))
        return rc, out, R.value
    import torch
    t = {k: None if v is None else torch.from_numpy(v.view(np.int64) if v.dtype == U64 else v).cuda() for k, v in out.items()}
    t_flat, t_offsets = torch.from_numpy(flat).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()
    rc = _lib.lib().msbwt_rle_read_overlaps_device(b._h, t_flat.data_ptr(), t_offsets.data_ptr(), n, m, M, strand, *[None if t[k] is None else t[k].data_ptr()
                                                                                                                  for k in ("offsets",) + COLUMNS],
                                                   capacity or 0, where_total, *[None if t[k] is None else t[k].data_ptr() for k in ("matched", "edges", "stops")],
                                                   torch.cuda.current_stream().cuda_stream)
    back = {k: None if v is None else (v.cpu().numpy().view(U64) if v.dtype == torch.int64 else v.cpu().numpy()) for k, v in t.items()}
    return rc, back, R.value


def host(a):
    a = np.asarray(a.cpu().numpy() if hasattr(a, "data_ptr") else a)
    return a.view(U64) if a.dtype == np.int64 else a


def check(got, want, what, capacity=None):
    """every per-query output given, and the columns: R records of the oracle's, the sentinel behind them"""
    for name in PER_QUERY:
        g = got[name] if isinstance(got, dict) else getattr(got, name)
        if g is None:
            continue
        g, w = host(g), getattr(want, name)
        bad = np.flatnonzero(g != w)
        assert g.shape == w.shape and g.dtype == w.dtype and bad.size == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])
    for name in COLUMNS:
        g = got[name] if isinstance(got, dict) else getattr(got, name)
        if g is None:
            continue
        g, w = host(g), getattr(want, name)
        bad = np.flatnonzero(g[:want.total] != w)
        assert bad.size == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])
        if capacity is None:
            assert g.size == want.total, (what, name)
        else:
            assert g.size == capacity + TAIL and (g[want.total:] == SENTINEL).all(), (what, name, "written past R")


def check_info(b, want, n, pieces=1):
    info = b.overlap_info()
    assert (info["queries"], info["symbols"], info["records"], info["edges"]) == (n, int(want.matched.sum()), want.total, int(want.edges.sum())), info
    assert (info["end"], info["empty"], info["bad_symbol"]) == tuple(int((want.stops == c).sum()) for c in (O.END, O.EMPTY, O.BAD_SYMBOL)), info
    assert info["pieces"] == pieces, info
    return info


def both_forms(b, queries, want, m, M, strand, what):
    """a filling call of exactly R records and a counting call, in the host form and in the device form"""
    n = len(queries[1]) - 1 if isinstance(queries, tuple) else len(queries)
    for device in (False, True):
        rc, got, R = raw(b, queries, m, M, strand, capacity=want.total, device=device)
        assert (rc, R) == (0, want.total), (what, device, rc, _lib.lib().msbwt_rle_last_error(b._h))
        check(got, want, (what, "device" if device else "host"), capacity=want.total)
        filled = check_info(b, want, n)
        rc, counted, R = raw(b, queries, m, M, strand, device=device)
        assert (rc, R) == (0, want.total)
        check(counted, want, (what, "counting", device))
        info = check_info(b, want, n)
        # at most two lines a step, and one more a bound in an OVERFLOW run block; a filling call searches twice
        per_step = 4 if b.get_block_format() == "runs" else 2
        assert info["lines"] <= per_step * int(want.matched.sum()) and filled["lines"] == (2 if want.total else 1) * info["lines"], (info, filled)
    b.device_status(0)


# ---- 1. ragged read sets: the oracle, and the string comparison through overlap_edges ----

_sets = {}


def ragged_index(orc, seed):
    """(reads, sorted reads, RleBWT built by the library, Decoded, queries as strings): computed once per seed"""
    if seed not in _sets:
        reads, genome = overlap_read_set(seed)
        rle = msbwt.RleBWT(device=0).build_from_reads(reads, ascii=True)
        rng = np.random.default_rng(seed)
        queries = list(reads)
        queries += ["".join(rng.choice(list("ACGTN"), size=int(rng.integers(0, 30)), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for _ in range(40)]
        for _ in range(60):
            at, length = int(rng.integers(0, len(genome) - 60)), int(rng.integers(1, 60))
            queries.append(genome[at:at + length])
        _sets[seed] = (reads, sorted(reads), rle, O.Decoded(orc.decompress(rle)), queries)
    return _sets[seed]


@pytest.mark.parametrize("seed", [0, 1])
def test_ragged_sets(orc, seed):
    import torch
    reads, ordered, rle, index, queries = ragged_index(orc, seed)
    assert np.array_equal(rle, orc.convert_to_vec(orc.naive_bwt(reads)))
    b = loaded(rle)
    held = b.device_bytes()
    coded = [codes_of(q) for q in queries]
    for m in (1, 5, 20):
        for M in (0, 10):
            for strand in (0, 1):
                want = O.Expected(index, coded, m, M, strand)
                both_forms(b, coded, want, m, M, strand, (seed, m, M, strand))
                assert b.device_bytes() == held
    # the mirror: strings in, numpy out; tensors in, tensors out
    want = O.Expected(index, coded, 5, 0, 1)
    assert want.total > 50 and (want.counts > 1).any()
    got = b.read_overlaps(queries, 5, strand=1, ascii=True)
    check(got, want, "mirror")
    assert np.array_equal(got.query_lengths, [len(q) for q in queries])
    counted = b.read_overlaps(queries, 5, strand=1, ascii=True, records=False)
    check(counted, want, "mirror, counting")
    assert counted.lengths is None
    flat, offsets = ragged(coded)
    t_got = b.read_overlaps_device(torch.from_numpy(flat).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda(), 5, strand=1)
    check(t_got, want, "mirror, tensors")
    # every edge the string comparison finds, and no other
    for m, M, strand in ((5, 0, 0), (5, 0, 1), (1, 10, 0)):
        res = b.read_overlaps(queries, m, max_overlap=M, strand=strand, ascii=True)
        edges = msbwt.overlap_edges(res, drop_self=False)
        assert edges.dtype == U64 and {tuple(int(x) for x in e) for e in edges} == O.edges_by_strings(queries, ordered, m, M, strand), (m, M, strand)
        assert len(edges) == int(res.edges.sum())
    # the queries that are reads of the index, under their ids: self edges dropped, then containments
    ids = np.array([ordered.index(r) for r in reads], dtype=U64)  # (a duplicate: its first copy)
    res = b.read_overlaps(reads, 1, ascii=True)
    every = {tuple(int(x) for x in e) for e in msbwt.overlap_edges(res, drop_self=False)}
    assert every == O.edges_by_strings(reads, ordered, 1)
    no_self = {tuple(int(x) for x in e) for e in msbwt.overlap_edges(res, query_ids=ids)}
    assert no_self == every - {(i, int(ids[i]), len(r)) for i, r in enumerate(reads)} and len(no_self) == len(every) - sum(len(r) > 0 for r in reads)
    proper = {tuple(int(x) for x in e) for e in msbwt.overlap_edges(res, query_ids=ids, drop_contained=True)}
    assert proper == {e for e in every if e[2] != len(reads[e[0]])} and proper < no_self


# ---- 2. both bounds in one block, and in two; 11. the round trip from extract_reads ----

_big = {}


def big_set():
    """4 000 reads of 40 bp from both strands of a 2 000-bp genome: (reads as a matrix of codes, in sorted order; rle built by the library; Decoded)"""
    if not _big:
        rng = np.random.default_rng(40)
        genome = np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=2000)]
        starts = rng.integers(0, 2000 - 40, size=4000)
        reads = np.stack([genome[s:s + 40] for s in starts])
        reads[1::2] = np.array(O.COMPLEMENT, dtype=np.uint8)[reads[1::2, ::-1]]  # every second read from the other strand
        reads = reads[np.lexsort(reads.T[::-1])]
        rle = msbwt.RleBWT(device=0).build_from_reads((reads.reshape(-1), np.arange(4001, dtype=U64) * U64(40)))
        _big.update(reads=reads, rle=rle, index=O.Decoded(msbwt.rle_bwt.rle_decode(rle)), want={})
    return _big


def big_expected(strand):
    s = big_set()
    if strand not in s["want"]:
        s["want"][strand] = O.Expected(s["index"], list(s["reads"]), 12, 0, strand)
    return s["want"][strand]


@pytest.mark.parametrize("blocks", ["planes", "runs"])
def test_bounds_in_one_block_and_in_two(blocks):
    s = big_set()
    index, reads = s["index"], s["reads"]
    assert index.T == 4000 * 41 and index.T // 256 == 640
    shift = 8 if blocks == "planes" else 9
    trace = []
    for q in reads[::50]:
        O.search(index, q, 12, trace=trace)
    inside = [(l, h) for _, l, h in trace if h < index.T]
    assert any(l >> shift == h >> shift for l, h in inside) and any(l >> shift != h >> shift for l, h in inside)
    b = loaded(s["rle"], block_format=blocks)
    assert b.get_block_format() == blocks
    queries = (reads.reshape(-1), np.arange(4001, dtype=U64) * U64(40))
    want = big_expected(0)
    assert want.total > 4000 and (want.stops == O.END).all() and (want.matched == 40).all()
    both_forms(b, queries, want, 12, 0, 0, blocks)
    # some steps stand in one block: fewer lines than two a step
    assert b.overlap_info()["lines"] < 2 * 4000 * 40


@pytest.mark.parametrize("strand", [0, 1])
def test_round_trip_from_extract_reads(strand):
    s = big_set()
    b = loaded(s["rle"])
    symbols, offsets = b.extract_reads(max_len=40)
    assert np.array_equal(symbols.reshape(4000, 40), s["reads"])
    b.set_overlap_piece(1500)  # three pieces: the base is carried from piece to piece
    res = b.read_overlaps((symbols, offsets), 12, strand=strand)
    check(res, big_expected(strand), ("round trip", strand))
    assert b.overlap_info()["pieces"] == 3 and b.overlap_info()["records"] == big_expected(strand).total
    edges = msbwt.overlap_edges(res, query_ids=np.arange(4000))
    # the string comparison: read r begins with the last j symbols of the query searched
    text = ["".join(LETTER[c] for c in r) for r in s["reads"]]
    sample = list(range(0, 4000, 100))
    want = O.edges_by_strings([text[i] for i in sample], text, 12, 0, strand)
    want = {(sample[q], r, j) for q, r, j in want} - ({(i, i, 40) for i in sample} if strand == 0 else set())
    rows = edges[np.isin(edges[:, 0], sample)]
    assert {tuple(int(x) for x in e) for e in rows} == want and len(want) > len(sample)
    if strand == 0:
        assert not ((edges[:, 0] == edges[:, 1]) & (edges[:, 2] == 40)).any()


# ---- 3. random streams that are no BWT ----

STREAMS = {
    "ones": lambda: random_stream(3, 3000, "ones"),              # single-symbol runs: every run block overflows
    "short": lambda: random_stream(4, 1500, "short"),
    "long": lambda: random_stream(5, 14, "long"),                # runs that span many blocks
    "mixed": lambda: random_stream(6, 40, "mixed"),              # 1-, 2- and 3-byte runs
    "leading dollars": lambda: np.concatenate([runs_to_bytes([0], [40000]), random_stream(8, 900, "short")]),
    "dense then long": lambda: np.concatenate([random_stream(9, 2000, "ones"), runs_to_bytes([2, 0, 5], [70000, 1200, 33000]), random_stream(10, 1500, "ones")]),
    "no dollar": lambda: random_stream(7, 900, "short", alphabet=(1, 2, 3, 4, 5)),
    "one symbol": lambda: runs_to_bytes([3], [1]),
}


@pytest.mark.parametrize("blocks", ["planes", "runs"])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_random_streams(orc, name, blocks):
    rle = STREAMS[name]()
    b, index = loaded(rle, block_format=blocks), O.Decoded(orc.decompress(rle))
    assert b.get_block_format() == blocks and b.get_total_size() == index.T
    rng = np.random.default_rng(11)
    queries = [rng.integers(1, 6, size=int(rng.integers(0, 14))).astype(np.uint8) for _ in range(300)]
    for m, M, strand in ((1, 0, 0), (1, 0, 1), (3, 7, 0)):
        want = O.Expected(index, queries, m, M, strand)
        both_forms(b, queries, want, m, M, strand, (name, blocks, m, M, strand))
    if name == "no dollar":
        assert want.total == 0
    if name in ("ones", "dense then long", "leading dollars"):
        assert want.total > 0


# ---- 4. every index form gives the same bytes ----

def test_every_index_form_gives_the_same_bytes(monkeypatch):
    s = big_set()
    queries = (s["reads"][::4].reshape(-1).copy(), np.arange(1001, dtype=U64) * U64(40))
    want = O.Expected(s["index"], list(s["reads"][::4]), 12, 0, 1)
    first = None
    forms = dict(ALL_FORMS, **{"host build": dict(), "host build, run blocks": dict(block_format="runs")})
    for form, knobs in forms.items():
        if form.startswith("host build"):
            monkeypatch.setenv("MSBWT_BUILD", "host")
        b = loaded(s["rle"], **knobs)
        rc, got, R = raw(b, queries, 12, 0, 1, capacity=want.total)
        assert (rc, R) == (0, want.total), form
        check(got, want, form, capacity=want.total)
        first = first or got
        assert all(np.array_equal(first[k], got[k]) for k in first), form


# ---- 5. batch shapes, pieces, odd addresses ----

def test_batch_shapes_and_pieces(orc):
    import torch
    rng = np.random.default_rng(21)
    genome = "".join(rng.choice(list("ACGT"), size=400))
    reads = [genome[int(a):int(a) + int(k)] for a, k in zip(rng.integers(0, 320, size=120), rng.integers(0, 81, size=120))]
    rle = msbwt.RleBWT(device=0).build_from_reads(reads, ascii=True)
    b, index = loaded(rle), O.Decoded(orc.decompress(rle))
    lengths = (0, 1, 7, 8, 9, 65)
    pool = [codes_of(genome[int(a):int(a) + k]) for k in lengths for a in rng.integers(0, 330, size=6)]
    for n in (1, 2, 3, 4, 5, 9, 33):
        queries = [pool[int(i)] for i in rng.permutation(len(pool))[:n]] if n < 33 else pool[:33]
        for strand in (0, 1):
            want = O.Expected(index, queries, 3, 0, strand)
            for piece in (1, 3, 7, n):
                b.set_overlap_piece(piece)
                pieces = -(-n // piece)
                for lead in (0, 1, 3):  # the first query starts `lead` bytes into an array that itself starts at an odd address
                    flat, offsets = ragged(queries)
                    backing = np.full(flat.size + lead + 1, 6, dtype=np.uint8)
                    backing[1 + lead:1 + lead + int(offsets[-1])] = flat[:int(offsets[-1])]
                    odd = (backing[1:], offsets + U64(lead))
                    assert odd[0].ctypes.data % 2 == 1
                    rc, got, R = raw(b, odd, 3, 0, strand, capacity=want.total)
                    assert (rc, R) == (0, want.total), (n, piece, lead)
                    check(got, want, (n, strand, piece, lead), capacity=want.total)
                    info = check_info(b, want, n, pieces)
                    largest = max(int(offsets[min(i + piece, n)] - offsets[i]) for i in range(0, n, piece))
                    assert info["piece_symbols"] == largest and info["scratch_bytes"] == msbwt.overlap_plan(n, True, piece, largest, info["piece_records"])
                    rc, counted, R = raw(b, odd, 3, 0, strand)
                    assert (rc, R) == (0, want.total) and all(np.array_equal(counted[k], got[k]) for k in PER_QUERY)
                    assert b.overlap_info()["piece_records"] == 0 and b.overlap_info()["scratch_bytes"] == msbwt.overlap_plan(n, True, piece, largest, 0)
                # the device form: tensors that start three bytes into their allocation
                flat, offsets = ragged(queries)
                t_backing = torch.full((flat.size + 3,), 6, dtype=torch.uint8, device="cuda")
                t_backing[3:] = torch.from_numpy(flat).cuda()
                res = b.read_overlaps_device(t_backing[3:], torch.from_numpy(offsets.view(np.int64)).cuda(), 3, strand=strand)
                b.device_status(torch.cuda.current_stream().cuda_stream)
                check(res, want, (n, strand, piece, "device"))
                info = check_info(b, want, n, pieces)
                assert info["scratch_bytes"] == msbwt.overlap_plan(n, False, piece) and info["piece_symbols"] == info["piece_records"] == 0
    b.set_overlap_piece(0)
    with pytest.raises(MsbwtError):
        b.set_overlap_piece((1 << 28) + 1)


# ---- 6. the capacity contract ----

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacity_contract(orc, device):
    reads, ordered, rle, index, queries = ragged_index(orc, 0)
    b = loaded(rle)
    coded = [codes_of(q) for q in queries]
    want = O.Expected(index, coded, 3)
    R = want.total
    assert R > 100
    for piece in (0, 50):
        b.set_overlap_piece(piece)
        for capacity in (R, R + 5):
            rc, got, total = raw(b, coded, 3, capacity=capacity, device=device)
            assert (rc, total) == (0, R)
            check(got, want, (piece, capacity), capacity=capacity)
        # one short: the error names R, the per-query outputs are written, nothing past the capacity
        rc, got, total = raw(b, coded, 3, capacity=R - 1, device=device)
        assert rc == _lib.ERR_INVALID_ARG and total == R and ("R = %d " % R) in _lib.lib().msbwt_rle_last_error(b._h).decode()
        for name in PER_QUERY:
            assert np.array_equal(got[name], getattr(want, name)), name
        for name in COLUMNS:
            assert (got[name][R - 1:] == SENTINEL).all(), name
        check_info(b, want, len(coded), pieces=-(-len(coded) // (piece or len(coded))))
        rc, got, total = raw(b, coded, 3, capacity=0, device=device)
        assert rc == _lib.ERR_INVALID_ARG and total == R and all((got[name] == SENTINEL).all() for name in COLUMNS)
    # only some of the per-query outputs, and none of them
    for keep in (("offsets",), ("stops", "edges"), ()):
        rc, got, total = raw(b, coded, 3, capacity=R, device=device, want=keep)
        assert (rc, total) == (0, R)
        check(got, want, keep, capacity=R)
    with pytest.raises(MsbwtError) as e:
        import torch
        flat, offsets = ragged(coded)
        b.read_overlaps_device(torch.from_numpy(flat).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda(), 3, capacity=R - 1)
    assert e.value.code == _lib.ERR_INVALID_ARG and e.value.records == R


# ---- 7. BAD_SYMBOL ----

def test_bad_symbols(orc):
    import torch
    reads, ordered, rle, index, queries = ragged_index(orc, 1)
    b = loaded(rle)
    coded = [codes_of(q) for q in queries[:80] if len(q) >= 12]
    assert len(coded) > 20
    for at, code in ((3, 0), (7, 6), (11, 255)):
        coded[at] = coded[at].copy()
        coded[at][len(coded[at]) // 2] = code
    coded[15] = np.array([6], dtype=np.uint8)
    for strand in (0, 1):
        want = O.Expected(index, coded, 1, 0, strand)
        bad = int((want.stops == O.BAD_SYMBOL).sum())  # (the other strand of a read may be EMPTY before it comes to the bad symbol)
        assert (bad == 4 if strand == 0 else bad >= 1) and want.stops[15] == O.BAD_SYMBOL and want.matched[15] == 0
        if strand == 0:
            assert any(want.offsets[i + 1] > want.offsets[i] for i in (3, 7, 11))  # records before the bad symbol stand
        rc, got, R = raw(b, coded, 1, 0, strand, capacity=want.total)
        assert rc == _lib.ERR_INVALID_SYMBOL and R == want.total
        check(got, want, ("bad symbols", strand), capacity=want.total)
        assert check_info(b, want, len(coded))["bad_symbol"] == bad
        rc, got, R = raw(b, coded, 1, 0, strand, capacity=want.total, device=True)
        assert rc == 0 and R == want.total
        check(got, want, ("bad symbols, device", strand), capacity=want.total)
        with pytest.raises(MsbwtError) as e:
            b.device_status(torch.cuda.current_stream().cuda_stream)
        assert e.value.code == _lib.ERR_INVALID_SYMBOL
        b.device_status(torch.cuda.current_stream().cuda_stream)  # read and cleared
    with pytest.raises(MsbwtError) as e:
        b.read_overlaps(coded, 1)
    assert e.value.code == _lib.ERR_INVALID_SYMBOL
    # offsets that decrease: the host form refuses them before anything runs, the device form flags them and searches an empty query
    flat, offsets = ragged(coded[16:21])  # (none of them holds a bad symbol)
    offsets[2] = offsets[1] - U64(1)
    rc, got, R = raw(b, (flat, offsets), 1)
    assert rc == _lib.ERR_INVALID_RANGE and R == 99 and all((got[k] == SENTINEL).all() for k in PER_QUERY)
    rc, got, R = raw(b, (flat, offsets), 1, device=True)
    assert rc == 0 and got["stops"][1] == O.END and got["matched"][1] == 0
    with pytest.raises(MsbwtError) as e:
        b.device_status(0)
    assert e.value.code == _lib.ERR_INVALID_RANGE


# ---- 8. the guards on a loaded index, in their order ----

def test_guards_on_a_loaded_index_in_their_order(orc):
    import torch
    lib = _lib.lib()
    reads, ordered, rle, index, queries = ragged_index(orc, 0)
    b = loaded(rle)
    flat, offsets = ragged([codes_of(q) for q in queries[:4]])
    b.read_overlaps((flat, offsets), 1)
    before, held = b.overlap_info(), b.device_bytes()
    assert before["queries"] == 4
    out = np.full(16, SENTINEL, dtype=U64)
    d_flat, d_offsets = torch.from_numpy(flat).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()
    d_out = torch.full((16,), SENTINEL, dtype=torch.int64, device="cuda")
    R = C.c_uint64(99)
    stream = torch.cuda.current_stream().cuda_stream
    decreasing = offsets.copy()
    decreasing[1] = decreasing[2] + U64(1)
    BIG = 2 ** 40

    def call(form, reads=True, offs=True, n=4, m=1, strand=0, columns=(False, False, False), total=True, off=None):
        where = C.byref(R) if total else None
        if form == "host":
            cols = [_ptr(out) if c else None for c in columns]
            return lib.msbwt_rle_read_overlaps(b._h, _ptr(flat) if reads else None, _ptr(offsets if off is None else off) if offs else None, n, m, 0, strand, _ptr(out),
                                               *cols, 16, where, None, None, None)
        cols = [d_out.data_ptr() if c else None for c in columns]
        return lib.msbwt_rle_read_overlaps_device(b._h, d_flat.data_ptr() if reads else None, d_offsets.data_ptr() if offs else None, n, m, 0, strand, d_out.data_ptr(),
                                                  *cols, 16, where, None, None, None, stream)

    for form in ("host", "device"):
        # the call's own arguments first, whatever else is wrong with it
        for bad in (dict(reads=False), dict(offs=False), dict(total=False), dict(m=0), dict(strand=2), dict(strand=-1), dict(columns=(True, False, False)),
                    dict(columns=(True, True, False)), dict(columns=(False, True, True))):
            for n in (4, BIG):
                assert call(form, n=n, off=decreasing, **bad) == _lib.ERR_INVALID_ARG, (form, bad, n)
        assert b"min_overlap" in (call(form, m=0) and lib.msbwt_rle_last_error(b._h))
        assert b"columns" in (call(form, columns=(True, False, True)) and lib.msbwt_rle_last_error(b._h))
        # n from 2^40 on, before an offset is read
        for n in (BIG, BIG + 5, 2 ** 63):
            assert call(form, n=n, off=decreasing) == _lib.ERR_TOO_LARGE, (form, n)
            assert b"2^40" in lib.msbwt_rle_last_error(b._h)
        assert (out == SENTINEL).all() and bool((d_out == SENTINEL).all()) and R.value == 99
        assert b.overlap_info() == before and b.device_bytes() == held
    # host form only: offsets that decrease, then the symbols
    assert call("host", off=decreasing) == _lib.ERR_INVALID_RANGE and b"decrease" in lib.msbwt_rle_last_error(b._h)
    far = offsets.copy()
    far[4] = far[0] + U64(BIG)
    assert call("host", off=far) == _lib.ERR_TOO_LARGE
    far[2] = far[1] - U64(1)
    assert call("host", off=far) == _lib.ERR_INVALID_RANGE
    assert (out == SENTINEL).all() and R.value == 99 and b.overlap_info() == before
    b.device_status(stream)  # nothing was flagged: nothing ran
    # NULL reads are no fault of a call of no queries
    assert call("host", reads=False, offs=False, n=0) == 0 and R.value == 0 and out[0] == 0 and (out[1:] == SENTINEL).all()
    assert lib.msbwt_rle_set_overlap_piece(b._h, 2 ** 28 + 1) == _lib.ERR_INVALID_ARG and lib.msbwt_rle_set_overlap_piece(b._h, 2 ** 28) == 0
    assert lib.msbwt_rle_set_overlap_piece(b._h, 0) == 0


# ---- 9. the empty batch and the empty index ----

def test_empty_batch_and_empty_index(orc):
    queries = [codes_of("ACGT"), codes_of(""), np.array([6, 1], dtype=np.uint8)]
    b = msbwt.RleBWT(device=0)
    b.load_vector(np.empty(0, dtype=np.uint8))
    want = O.Expected(O.Decoded([]), queries, 1)
    assert want.total == 0 and (want.stops == O.EMPTY).all()
    for device in (False, True):
        rc, got, R = raw(b, queries, 1, capacity=4, device=device)
        assert (rc, R) == (0, 0)
        check(got, want, ("empty index", device), capacity=4)
        info = b.overlap_info()
        assert (info["queries"], info["empty"], info["scratch_bytes"], info["pieces"], info["lines"]) == (3, 3, 0, 0, 0)
    b.load_vector(runs_to_bytes([0, 1], [2, 2]))
    for device in (False, True):
        rc, got, R = raw(b, [], 1, capacity=4, device=device)
        assert (rc, R) == (0, 0) and got["offsets"].tolist() == [0] and all((got[c] == SENTINEL).all() for c in COLUMNS)
        info = b.overlap_info()
        assert (info["queries"], info["scratch_bytes"], info["pieces"]) == (0, 0, 0)
    res = b.read_overlaps([], 1)
    assert res.offsets.tolist() == [0] and res.lengths.size == 0 and msbwt.overlap_edges(res).shape == (0, 3)
    b.load_vector(runs_to_bytes([1, 0], [2, 2]))  # AA$$: the BWT of the reads A and A
    res = b.read_overlaps(["A", "CA", ""], 1, ascii=True)
    assert (res.offsets.tolist(), res.lengths.tolist(), res.first.tolist(), res.counts.tolist()) == ([0, 1, 2, 2], [1, 1], [0, 0], [2, 2])
    assert (res.matched.tolist(), res.edges.tolist(), res.stops.tolist()) == ([1, 1, 0], [2, 2, 0], [O.END, O.EMPTY, O.END])


# ---- 10. beyond 2^32 ----

def wide_runs():
    """about 1.3e10 rows in a few hundred bytes of RLE: a leading '$' run and, inside the rows of the A block, a second one, each longer
    than 2^32, so that a range, a record's first read and a record's count all exceed 32 bits"""
    rng = np.random.default_rng(33)
    a, c = (1 << 32) + 1000, (1 << 32) + 500

    def short(n, alphabet):
        syms = np.zeros(n, dtype=np.int64)
        syms[0] = alphabet[0]
        for i in range(1, n):
            syms[i] = alphabet[int(rng.integers(0, len(alphabet)))]
            while syms[i] == syms[i - 1]:
                syms[i] = alphabet[int(rng.integers(0, len(alphabet)))]
        return syms, rng.integers(1, 300, size=n)

    s1, l1 = short(200, (2, 3, 5, 1, 4))
    s2, l2 = short(300, (2, 0, 3, 5, 1, 4))
    l2 = np.where(s2 == 0, np.minimum(l2, 9), l2)
    if s2[-1] == 1:
        s2[-1] = 3 if s2[-2] != 3 else 2
    syms = np.concatenate([[0, 1], s1, [0], s2, [1, 5, 2]])
    lens = np.concatenate([[a, c + 2000], l1, [c], l2, [100000, 1 << 27, 77]])
    keep = np.concatenate([[True], syms[1:] != syms[:-1]])
    assert keep.all()
    return syms, lens


@pytest.mark.parametrize("blocks", ["planes", "runs"])
def test_ranges_and_records_past_32_bits(blocks):
    import torch
    syms, lens = wide_runs()
    index = O.Runs(syms, lens)
    edge = 1 << 32
    assert index.T > 3 * edge
    rng = np.random.default_rng(5)
    queries = [np.array(q, dtype=np.uint8) for q in ([1], [2, 1], [3, 1], [5, 1], [1, 1], [2], [5], [5, 5, 5])]
    queries += [rng.integers(1, 6, size=int(rng.integers(1, 7))).astype(np.uint8) for _ in range(120)]
    want = O.Expected(index, queries, 1)
    trace = []
    for q in queries:
        O.search(index, q, 1, trace=trace)
    assert ((want.first > U64(edge)) & (want.counts > U64(edge))).any() and any(l > edge and h - l > edge for _, l, h in trace) and (want.matched > 2).any()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device("cuda", 0))
    if free < 16e9:
        pytest.skip("needs 16 GB of free HBM")
    b = msbwt.RleBWT(device=0)
    b.set_block_format(blocks)
    b.set_pair_index(0)
    b.set_sparse_table(0)
    b.load_vector(runs_to_bytes(syms, lens))
    assert b.get_total_size() == index.T and b.get_block_format() == blocks
    print("%s blocks of %d rows: device_bytes() = %.2f GB" % (blocks, index.T, b.device_bytes() / 1e9))
    for strand in (0, 1):
        want = O.Expected(index, queries, 1, 0, strand)
        both_forms(b, queries, want, 1, 0, strand, (blocks, strand))
