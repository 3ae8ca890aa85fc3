"""Left walks on the device (include/msbwt_hip.h, "left walks": msbwt_rle_walk_rows[_device], msbwt_rle_extract_reads[_device]) against
tests/walk_oracle.py, which knows the BWT string alone: ragged read sets at every packing border, random RLE streams of every kind,
batch shapes and pieces, every index form, the extraction round trip and its capacity contract, truncation, locate_kmer against string
search, and rows past 2^32 against the closed form over a run list."""
import ctypes as C
import importlib

import numpy as np
import pytest

import walk_oracle as W
from rle_random import random_stream, runs_to_bytes
from test_gpu_kmer_graph import FORMS
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_spectrum import loaded

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
SENTINEL = 0xEE
NAMES = ("symbols", "steps", "stops", "last", "reads")
ALL_FORMS = dict(FORMS, **{"no sparse table": dict(sparse_table=0)})
LETTER = "$ACGNT"


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_walk(b, rows, max_steps, want=(True,) * 5):
    """msbwt_rle_walk_rows itself -> (return code, the five arrays; None where `want` says NULL); the rows of symbols pre-filled"""
    rows = np.ascontiguousarray(rows, dtype=U64)
    n = len(rows)
    arrays = [np.full((n, max_steps), SENTINEL, dtype=np.uint8), np.full(n, 77, dtype=U64), np.full(n, 77, dtype=np.uint8), np.full(n, 77, dtype=U64),
              np.full(n, 77, dtype=U64)]
    arrays = [a if w else None for a, w in zip(arrays, want)]
    rc = _lib.lib().msbwt_rle_walk_rows(b._h, _ptr(rows), n, max_steps, *[_ptr(a) for a in arrays])
    return rc, arrays


def check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        g = np.asarray(g.cpu().numpy() if hasattr(g, "data_ptr") else g)
        g = g.view(U64) if g.dtype == np.int64 else g
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert g.shape == w.shape and bad.size == 0, (what, name, bad[:5], g[bad[:3]], w[bad[:3]])


def check_info(b, want, pieces=1):
    info = b.walk_info()
    steps, stops = want[1], want[2]
    assert info["walks"] == len(steps) and info["steps"] == int(steps.sum()) and info["pieces"] == (pieces if len(steps) else 0), info
    assert (info["dollar"], info["max_steps"], info["bad_row"]) == tuple(int((stops == c).sum()) for c in (W.DOLLAR, W.MAX_STEPS, W.BAD_ROW)), info
    return info


# ---- 1. ragged read sets: every row, every packing border, every output NULL in turn, all three forms ----

@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets(orc, seed):
    import torch
    reads = ragged_set(seed)
    rle = naive_rle(orc, reads)
    b, index = loaded(rle), W.Decoded(orc.decompress(rle))
    held = b.device_bytes()
    rows = np.arange(index.T, dtype=U64)
    dev = torch.device("cuda", 0)
    for max_steps in (0, 1, 3, 4, 5, 7, 8, 9, 200):
        want = W.expected_arrays(index, rows, max_steps, fill=SENTINEL)
        # the host form through the mirror, rows pre-filled with the sentinel
        symbols = np.full((len(rows), max_steps), SENTINEL, dtype=np.uint8)
        got = b.walk_rows(rows, max_steps, symbols=symbols)
        assert got[0] is symbols and [g.dtype for g in got] == [np.uint8, U64, np.uint8, U64, U64]
        check(got, want, (seed, max_steps, "host"))
        info = check_info(b, want)
        assert info["scratch_bytes"] == msbwt.walk_plan(len(rows), max_steps, symbols=True, host=True) and b.device_bytes() == held
        # locate: no symbols
        located = b.locate_rows(rows, max_steps)
        check((None, located[1], located[2], None, located[0]), want, (seed, max_steps, "locate"))
        assert b.walk_info()["scratch_bytes"] == msbwt.walk_plan(len(rows), max_steps, symbols=False, host=True)
        # torch tensors: the device form; the rows of symbols start at an odd address
        backing = torch.full((len(rows) * max_steps + 3,), SENTINEL, dtype=torch.uint8, device=dev)
        t_symbols = backing[3:].view(len(rows), max_steps)
        t_got = b.walk_rows(torch.from_numpy(rows.view(np.int64)).to(dev), max_steps, symbols=t_symbols)
        b.device_status(torch.cuda.current_stream(dev).cuda_stream)
        check(t_got, want, (seed, max_steps, "device"))
        assert (backing[:3].cpu().numpy() == SENTINEL).all()
        info = check_info(b, want)
        assert info["scratch_bytes"] == 256 == msbwt.walk_plan(len(rows), max_steps, host=False) and b.device_bytes() == held
    # every output NULL in turn, and all of them
    want = W.expected_arrays(index, rows, 9, fill=SENTINEL)
    for missing in list(range(5)) + [None]:
        mask = tuple(missing is not None and i != missing for i in range(5))
        rc, got = raw_walk(b, rows, 9, mask)
        assert rc == 0
        check(got, want, (seed, "NULL", missing))
        check_info(b, want)
    t_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
    for missing in range(5):
        outs = [torch.full((len(rows), 9), SENTINEL, dtype=torch.uint8, device=dev)] + [torch.zeros(len(rows), dtype=torch.uint8 if i == 2 else torch.int64, device=dev)
                                                                                      for i in range(1, 5)]
        outs[missing] = None
        b.walk_rows_device(t_rows.data_ptr(), len(rows), 9, *[None if t is None else t.data_ptr() for t in outs])
        b.device_status(0)
        check(outs, want, (seed, "device NULL", missing))
    # the sequences in reading order: the '$' rows give the sorted reads
    got = b.walk_rows(np.arange(len(reads), dtype=U64), 200)
    assert msbwt.walk_sequences(got[0], got[1], text=True) == sorted(reads)


# ---- 2. random RLE streams: any stream is walked by the definition; bad rows among good ones ----

STREAMS = {
    "ones": lambda: random_stream(3, 3000, "ones"),              # single-symbol runs: every run block overflows
    "short": lambda: random_stream(4, 1500, "short"),
    "long": lambda: random_stream(5, 14, "long"),
    "mixed": lambda: random_stream(6, 40, "mixed"),
    "no dollar": lambda: random_stream(7, 900, "short", alphabet=(1, 2, 3, 4, 5)),   # every walk ends at MAX_STEPS
    "dollars only": lambda: runs_to_bytes([0], [1500]),
    "one symbol": lambda: runs_to_bytes([3], [1]),
}


@pytest.mark.parametrize("blocks", ["planes", "runs"])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_random_streams(orc, name, blocks):
    rle = STREAMS[name]()
    b, index = loaded(rle, block_format=blocks), W.Decoded(orc.decompress(rle))
    assert b.get_block_format() == blocks and b.get_total_size() == index.T
    rows = np.concatenate([np.arange(index.T, dtype=U64), np.array([index.T - 1, index.T, 1 << 40, 2 ** 64 - 1, 0], dtype=U64)])
    for max_steps in (0, 6, 33):
        want = W.expected_arrays(index, rows, max_steps, fill=SENTINEL)
        rc, got = raw_walk(b, rows, max_steps)
        assert rc == _lib.ERR_INVALID_RANGE  # the three bad rows, as constrain_ranges reports a bad range; the others are answered
        check(got, want, (name, blocks, max_steps))
        check_info(b, want)
        rc, got = raw_walk(b, rows[:index.T], max_steps)
        assert rc == 0
        check(got, [w[:index.T] for w in want], (name, blocks, max_steps, "good rows only"))
    if name == "no dollar":
        assert (want[2][:index.T] == W.MAX_STEPS).all() and (want[1][:index.T] == 33).all()
    if name == "dollars only":
        assert (want[2][:index.T] == W.DOLLAR).all() and np.array_equal(want[4][:index.T], np.arange(index.T, dtype=U64))
    with pytest.raises(MsbwtError) as e:
        b.walk_rows(rows, 3)
    assert e.value.code == _lib.ERR_INVALID_RANGE


def test_bad_rows_in_the_device_form_show_in_device_status(orc):
    import torch
    rle = STREAMS["mixed"]()
    b, index = loaded(rle), W.Decoded(orc.decompress(rle))
    rows = np.array([5, index.T, 7, 1 << 40, index.T - 1], dtype=U64)
    got = b.walk_rows(torch.from_numpy(rows.view(np.int64)).cuda(), 12)
    check(got, W.expected_arrays(index, rows, 12), "device form")
    with pytest.raises(MsbwtError) as e:
        b.device_status(torch.cuda.current_stream().cuda_stream)
    assert e.value.code == _lib.ERR_INVALID_RANGE
    b.device_status(torch.cuda.current_stream().cuda_stream)  # read and cleared


# ---- 3. batch shapes and pieces ----

def test_batch_shapes_and_pieces(orc):
    rle = naive_rle(orc, ragged_set(2))
    b, index = loaded(rle), W.Decoded(orc.decompress(rle))
    rng = np.random.default_rng(3)
    for n in (1, 78):
        rows = rng.integers(0, index.T, size=n).astype(U64)
        check(b.walk_rows(rows, 40), W.expected_arrays(index, rows, 40), n)
        assert b.walk_info()["pieces"] == 1
    rows = rng.integers(0, index.T, size=1000).astype(U64)
    want = W.expected_arrays(index, rows, 21)
    whole = b.walk_rows(rows, 21)
    b.set_walk_piece(64)
    pieced = b.walk_rows(rows, 21)
    check(pieced, want, "pieces of 64")
    check_info(b, want, pieces=16)
    assert b.walk_info()["scratch_bytes"] == msbwt.walk_plan(1000, 21, piece=64) < msbwt.walk_plan(1000, 21)
    assert all(np.array_equal(x, y) for x, y in zip(whole, pieced))
    located = b.locate_rows(rows, 21)
    assert np.array_equal(located[0], want[4]) and np.array_equal(located[1], want[1])
    # more walks than the automatic piece holds
    b.set_walk_piece(0)
    rows = rng.integers(0, index.T, size=(1 << 20) + 77).astype(U64)
    want = W.expected_arrays(index, rows, 5)
    got = b.walk_rows(rows, 5)
    check(got, want, "two pieces at the default")
    check_info(b, want, pieces=2)
    b.set_walk_piece(1 << 21)
    one = b.walk_rows(rows, 5)
    assert b.walk_info()["pieces"] == 1 and all(np.array_equal(x, y) for x, y in zip(one, got))
    with pytest.raises(MsbwtError):
        b.set_walk_piece((1 << 28) + 1)


def test_empty_batch_and_empty_index():
    b = msbwt.RleBWT(device=0)
    b.load_vector(np.empty(0, dtype=np.uint8))
    rc, got = raw_walk(b, np.array([0, 1], dtype=U64), 4)
    assert rc == 0 and (got[0] == SENTINEL).all() and (got[2] == 77).all() and b.walk_info()["scratch_bytes"] == 0
    symbols, offsets = b.extract_reads()
    assert symbols.size == 0 and offsets.tolist() == [0]
    b.load_vector(runs_to_bytes([0, 1], [2, 2]))
    rc, got = raw_walk(b, np.empty(0, dtype=U64), 4)
    assert rc == 0 and b.walk_info() == dict(b.walk_info(), walks=0, steps=0, pieces=0, scratch_bytes=0)


def test_guards_on_a_loaded_index_in_their_order(orc):
    """NULL rows with n > 0 and max_len == 0 / a NULL total (INVALID_ARG) answer before the 2^40 limits (TOO_LARGE), those before the
    ids (INVALID_RANGE); a refused call writes nothing, leaves walk_info as it was and allocates nothing"""
    import torch
    lib = _lib.lib()
    reads = ragged_set(2)
    b = loaded(naive_rle(orc, reads))
    n_reads = len(reads)
    rows = np.array([0, 1], dtype=U64)
    b.walk_rows(rows, 3)
    before, held = b.walk_info(), b.device_bytes()
    assert before["walks"] == 2
    d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
    d_out = torch.full((64,), 77, dtype=torch.int64, device="cuda")
    steps = np.full(2, 77, dtype=U64)
    total, truncated = C.c_uint64(99), C.c_uint64(99)
    stream = torch.cuda.current_stream().cuda_stream
    BIG = 2 ** 40

    def walk(form, where, n, max_steps):
        if form == "host":
            return lib.msbwt_rle_walk_rows(b._h, _ptr(rows) if where else None, n, max_steps, None, _ptr(steps), None, None, None)
        return lib.msbwt_rle_walk_rows_device(b._h, d_rows.data_ptr() if where else None, n, max_steps, None, d_out.data_ptr(), None, None, None, stream)

    def extract(form, ids, first, n, max_len, out_total=True):
        where_total = C.byref(total) if out_total else None
        if form == "host":
            return lib.msbwt_rle_extract_reads(b._h, _ptr(rows) if ids else None, first, n, max_len, None, _ptr(steps), 0, where_total, C.byref(truncated))
        return lib.msbwt_rle_extract_reads_device(b._h, d_rows.data_ptr() if ids else None, first, n, max_len, None, d_out.data_ptr(), 0, where_total, C.byref(truncated), stream)

    for form in ("host", "device"):
        # walk_rows: NULL rows, then the limits
        for n, max_steps in ((2, 3), (2, BIG), (2 ** 39, 2)):
            assert walk(form, False, n, max_steps) == _lib.ERR_INVALID_ARG, (form, n, max_steps)
            assert b"null" in lib.msbwt_rle_last_error(b._h)
        for n, max_steps in ((2, BIG), (0, BIG), (2 ** 39 + 1, 2), (2 ** 20, 2 ** 20)):
            assert walk(form, True, n, max_steps) == _lib.ERR_TOO_LARGE, (form, n, max_steps)
            assert b"2^40" in lib.msbwt_rle_last_error(b._h)
        assert walk(form, False, 0, BIG) == _lib.ERR_TOO_LARGE  # NULL rows are no fault of a call of no walks
        # extract_reads: max_len == 0 and the NULL total first, then the limits, then the ids the host knows
        for ids, first, n, max_len, out_total in ((True, 0, 2, 0, True), (False, n_reads, 2 ** 39, 0, True), (True, 0, 2, BIG, False), (False, n_reads, 2, 5, False)):
            assert extract(form, ids, first, n, max_len, out_total) == _lib.ERR_INVALID_ARG, (form, ids, first, n, max_len, out_total)
        for ids, first, n, max_len in ((True, 0, 2, BIG), (False, n_reads, 2 ** 39 + 1, 2), (False, n_reads + 5, 2 ** 20, 2 ** 20)):
            assert extract(form, ids, first, n, max_len) == _lib.ERR_TOO_LARGE, (form, ids, first, n, max_len)
        for first, n in ((n_reads, 1), (n_reads - 1, 2), (0, n_reads + 1), (2 ** 63, 2)):
            assert extract(form, False, first, n, 5) == _lib.ERR_INVALID_RANGE, (form, first, n)
            assert b"reads of the index" in lib.msbwt_rle_last_error(b._h)
        assert (steps == 77).all() and total.value == truncated.value == 99 and bool((d_out == 77).all())
        assert b.walk_info() == before and b.device_bytes() == held
    # ids in a host array: refused on the host
    bad = np.array([0, n_reads], dtype=U64)
    assert lib.msbwt_rle_extract_reads(b._h, _ptr(bad), 0, 2, 5, None, _ptr(steps), 0, C.byref(total), None) == _lib.ERR_INVALID_RANGE
    assert (steps == 77).all() and total.value == 99 and b.walk_info() == before
    b.device_status(stream)  # nothing was flagged: nothing ran
    # the piece setter's own guard
    assert lib.msbwt_rle_set_walk_piece(b._h, 2 ** 28 + 1) == _lib.ERR_INVALID_ARG and lib.msbwt_rle_set_walk_piece(b._h, 2 ** 28) == 0
    assert lib.msbwt_rle_set_walk_piece(b._h, 0) == 0


# ---- 4. every index form ----

def test_every_index_form_gives_the_same_bytes(orc):
    _, rle = read_set("repeat_150")
    index = W.Decoded(orc.decompress(rle))
    rng = np.random.default_rng(9)
    rows = np.concatenate([np.arange(100, dtype=U64), rng.integers(0, index.T, size=3000).astype(U64)])
    want = W.expected_arrays(index, rows, 200, fill=SENTINEL)
    assert (want[2] == W.DOLLAR).all() and want[1].max() == 150
    first = None
    for form, knobs in ALL_FORMS.items():
        b = loaded(rle, **knobs)
        rc, got = raw_walk(b, rows, 200)
        assert rc == 0
        check(got, want, form)
        first = first or got
        assert all(np.array_equal(x, y) for x, y in zip(first, got)), form


# ---- 5. extraction ----

def ragged_of(symbols, offsets):
    return [bytes(symbols[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])]


@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_extraction_round_trip_on_ragged_sets(orc, seed):
    reads = ragged_set(seed)
    builder = msbwt.RleBWT(device=0)
    rle = builder.build_from_reads(reads, ascii=True)
    b, index = loaded(rle), W.Decoded(orc.decompress(rle))
    ordered = sorted(reads)
    symbols, offsets = b.extract_reads(max_len=80)
    assert symbols.dtype == np.uint8 and offsets.dtype == U64
    assert ["".join(LETTER[c] for c in r) for r in ragged_of(symbols, offsets)] == ordered
    want = W.extract(index, range(len(reads)), 80)
    assert np.array_equal(symbols, want[0]) and np.array_equal(offsets, want[1]) and want[2] == 0
    info = b.walk_info()
    assert (info["walks"], info["steps"], info["dollar"], info["max_steps"], info["bad_row"], info["pieces"]) == (len(reads), symbols.size, len(reads), 0, 0, 1)
    # the reads go back into the builder as they are
    assert np.array_equal(builder.build_from_reads((symbols, offsets)), rle)
    # ids shuffled, with repeats; slices; pieces
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(reads), size=3 * len(reads) + 1)
    for piece in (0, 7):
        b.set_walk_piece(piece)
        got = b.extract_reads(read_ids=ids, max_len=80)
        want = W.extract(index, ids, 80)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), piece
        for first, n in ((0, 1), (len(reads) - 1, 1), (len(reads) // 3, len(reads) // 2), (len(reads), 0)):
            got = b.extract_reads(first=first, n=n, max_len=80)
            want = W.extract(index, range(first, first + n), 80)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (piece, first, n)
        # truncated to the last 9 symbols
        got = b.extract_reads(max_len=9, truncate=True)
        want = W.extract(index, range(len(reads)), 9)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and b.walk_info()["max_steps"] == want[2] == sum(len(r) > 9 for r in reads)
    # ids out of range: refused on the host, nothing walked
    for bad in ([len(reads)], [0, 1 << 40]):
        with pytest.raises(MsbwtError) as e:
            b.extract_reads(read_ids=bad, max_len=80)
        assert e.value.code == _lib.ERR_INVALID_RANGE
    with pytest.raises(MsbwtError) as e:
        b.extract_reads(first=1, n=len(reads), max_len=80)
    assert e.value.code == _lib.ERR_INVALID_RANGE


def test_extraction_round_trip_on_4000_reads(orc):
    (flat, offsets), rle = read_set("plain_100")
    b = loaded(rle)
    b.set_walk_piece(1500)  # three pieces: the base is carried from piece to piece
    symbols, got_offsets = b.extract_reads(max_len=100)
    rows = flat.reshape(4000, 100)
    ordered = rows[np.lexsort(rows.T[::-1])]
    assert np.array_equal(got_offsets, offsets) and np.array_equal(symbols.reshape(4000, 100), ordered)
    assert b.walk_info()["pieces"] == 3 and b.walk_info()["steps"] == 400000
    assert np.array_equal(msbwt.RleBWT(device=0).build_from_reads((symbols, got_offsets)), rle)
    ids = np.random.default_rng(1).integers(0, 4000, size=5000)
    symbols, got_offsets = b.extract_reads(read_ids=ids, max_len=128)
    assert np.array_equal(symbols.reshape(5000, 100), ordered[ids]) and np.array_equal(got_offsets, np.arange(5001, dtype=U64) * U64(100))


def raw_extract(b, ids, first, n, max_len, capacity, symbols=True, offsets=True, device=False):
    """msbwt_rle_extract_reads[_device] itself -> (return code, symbols buffer of capacity + 16 sentinel bytes, offsets, S, truncated)"""
    import torch
    out_symbols = np.full(capacity + 16, SENTINEL, dtype=np.uint8) if symbols else None
    out_offsets = np.full(n + 1, 77, dtype=U64) if offsets else None
    total, truncated = C.c_uint64(99), C.c_uint64(99)
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=U64)
    if not device:
        rc = _lib.lib().msbwt_rle_extract_reads(b._h, _ptr(ids), first, n, max_len, _ptr(out_symbols), _ptr(out_offsets), capacity, C.byref(total), C.byref(truncated))
        return rc, out_symbols, out_offsets, total.value, truncated.value
    t_ids = None if ids is None else torch.from_numpy(ids.view(np.int64)).cuda()
    t_symbols = None if out_symbols is None else torch.from_numpy(out_symbols).cuda()
    t_offsets = None if out_offsets is None else torch.from_numpy(out_offsets.view(np.int64)).cuda()
    rc = _lib.lib().msbwt_rle_extract_reads_device(b._h, *[None if t is None else t.data_ptr() for t in (t_ids,)], first, n, max_len,
                                                   *[None if t is None else t.data_ptr() for t in (t_symbols, t_offsets)], capacity, C.byref(total), C.byref(truncated),
                                                   torch.cuda.current_stream().cuda_stream)
    return (rc, None if t_symbols is None else t_symbols.cpu().numpy(), None if t_offsets is None else t_offsets.cpu().numpy().view(U64), total.value, truncated.value)


def pad(x):
    return (x + 255) // 256 * 256


def extract_scratch(n, max_len, ids, symbols, offsets, host, piece=0):
    """the terms include/msbwt_hip.h states for the scratch of an extraction"""
    P = min(n, piece if piece else 2 ** 20)
    w, x = 1, P + 1
    while x > 2048:
        x = -(-x // 2048)
        w += x
    size = 256 + pad(8 * (P + 1)) + pad(8 * w) + (pad(P * max_len) if symbols else 0)
    if host:
        size += (pad(8 * P) if ids else 0) + (pad(8 * (P + 1)) if offsets else 0) + (pad(P * max_len) if symbols else 0)
    return size


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacity_contract(orc, device):
    reads = ragged_set(5)
    rle = naive_rle(orc, reads)
    b, index = loaded(rle), W.Decoded(orc.decompress(rle))
    held = b.device_bytes()
    n, max_len = len(reads), 80
    want_symbols, want_offsets, _ = W.extract(index, range(n), max_len)
    S = want_symbols.size
    assert 0 < S < n * max_len
    # lengths only
    rc, _, offsets, total, truncated = raw_extract(b, None, 0, n, max_len, 0, symbols=False, device=device)
    assert (rc, total, truncated) == (0, S, 0) and np.array_equal(offsets, want_offsets)
    assert b.walk_info()["pieces"] == 1 and b.walk_info()["scratch_bytes"] == extract_scratch(n, max_len, False, False, True, not device)
    rc, _, _, total, _ = raw_extract(b, None, 0, n, max_len, 0, symbols=False, offsets=False, device=device)
    assert (rc, total) == (0, S)
    assert b.walk_info()["pieces"] == 1 and b.walk_info()["scratch_bytes"] == extract_scratch(n, max_len, False, False, False, not device)
    # several pieces, with ids: the terms at P = 7, and both walks' pieces counted
    b.set_walk_piece(7)
    ids = np.arange(n, dtype=U64)[::-1].copy()
    for capacity, walks in ((n * max_len, 1), (n * max_len - 1, 2)):
        rc, symbols, _, total, _ = raw_extract(b, ids, 0, n, max_len, capacity, device=device)
        assert (rc, total) == (0, S) and np.array_equal(symbols[:S], W.extract(index, ids, max_len)[0])
        assert b.walk_info()["pieces"] == walks * -(-n // 7) and b.walk_info()["scratch_bytes"] == extract_scratch(n, max_len, True, True, True, not device, piece=7)
    b.set_walk_piece(0)
    # exact, above need (one walk: n x max_len fits) and in between (two walks): everything past S is untouched
    for capacity in (S, S + 5, n * max_len - 1, n * max_len, n * max_len + 1):
        rc, symbols, offsets, total, truncated = raw_extract(b, None, 0, n, max_len, capacity, device=device)
        assert (rc, total, truncated) == (0, S, 0), capacity
        assert np.array_equal(symbols[:S], want_symbols) and (symbols[S:] == SENTINEL).all() and np.array_equal(offsets, want_offsets), capacity
        info = b.walk_info()
        assert info["steps"] == S and b.device_bytes() == held
        # a capacity that cannot be short is walked once, a smaller one twice: the pieces launched say which
        assert info["pieces"] == (1 if capacity >= n * max_len else 2), (capacity, info)
        assert info["scratch_bytes"] == extract_scratch(n, max_len, ids=False, symbols=True, offsets=True, host=not device), (capacity, info)
    # one short: the error names S, the offsets and the bytes past the capacity are untouched
    rc, symbols, offsets, total, _ = raw_extract(b, None, 0, n, max_len, S - 1, device=device)
    assert rc == _lib.ERR_INVALID_ARG and total == S and str(S) in _lib.lib().msbwt_rle_last_error(b._h).decode()
    assert (offsets == 77).all() and (symbols[S - 1:] == SENTINEL).all()
    assert b.walk_info()["pieces"] == 1 and b.walk_info()["steps"] == S  # refused after the walk for the lengths
    # symbols without offsets
    rc, symbols, _, total, _ = raw_extract(b, None, 0, n, max_len, S, offsets=False, device=device)
    assert (rc, total) == (0, S) and np.array_equal(symbols[:S], want_symbols)
    # ids in the device form: a bad one shows in the flags and gets length 0
    if device:
        ids = np.array([1, n, 0, 1 << 40, 2], dtype=U64)
        rc, symbols, offsets, total, _ = raw_extract(b, ids, 0, len(ids), max_len, len(ids) * max_len, device=True)
        want = W.extract(index, [1, 0, 2], max_len)
        assert rc == 0 and total == want[0].size and np.array_equal(symbols[:total], want[0])
        assert np.array_equal(offsets, want[1][[0, 1, 1, 2, 2, 3]])
        with pytest.raises(MsbwtError) as e:
            b.device_status(0)
        assert e.value.code == _lib.ERR_INVALID_RANGE
        assert b.walk_info()["bad_row"] == 2


def test_truncation_and_one_long_walk(orc):
    rng = np.random.default_rng(12)
    read = "".join(rng.choice(list("ACGT"), size=5000))
    codes = np.array([LETTER.index(c) for c in read], dtype=np.uint8)
    b = msbwt.RleBWT(device=0)
    b.load_reads([read], ascii=True)
    rc, symbols, offsets, total, truncated = raw_extract(b, None, 0, 1, 100, 100)
    assert (rc, total, truncated) == (0, 100, 1) and np.array_equal(symbols[:100], codes[-100:]) and offsets.tolist() == [0, 100]
    with pytest.raises(MsbwtError):
        b.extract_reads(max_len=100)
    symbols, offsets = b.extract_reads(max_len=100, truncate=True)
    assert np.array_equal(symbols, codes[-100:]) and offsets.tolist() == [0, 100]
    # 5000 steps of one walk in one launch; at max_len == the length the read is whole
    symbols, offsets = b.extract_reads(max_len=5000)
    assert np.array_equal(symbols, codes) and offsets.tolist() == [0, 5000]
    assert b.walk_info()["steps"] == 5000 and b.walk_info()["max_steps"] == 0
    symbols, offsets = b.extract_reads(max_len=4999, truncate=True)
    assert np.array_equal(symbols, codes[1:]) and b.walk_info()["max_steps"] == 1


# ---- 6. locate_kmer against string search ----

@pytest.mark.parametrize("k", [1, 4, 17])
def test_locate_kmer_equals_string_search(orc, k):
    reads = ragged_set(1)
    b = loaded(naive_rle(orc, reads))
    ordered = sorted(reads)
    kmers = sorted({r[p:p + k] for r in reads for p in range(len(r) - k + 1)})
    assert kmers
    for q in kmers:
        want = sorted((i, p) for i, r in enumerate(ordered) for p in range(len(r) - k + 1) if r[p:p + k] == q)
        got_reads, got_offsets = b.locate_kmer(np.array([LETTER.index(c) for c in q], dtype=np.uint8), 80)
        assert list(zip(got_reads.tolist(), got_offsets.tolist())) == want, q
    got_reads, got_offsets = b.locate_kmer(np.array([4] * 9, dtype=np.uint8), 80)  # NNNNNNNNN does not occur
    assert got_reads.size == 0 and got_offsets.size == 0
    # offsets beyond max_steps are not found: the mirror says so
    longest = max(reads, key=len)
    if len(longest) >= k + 5:
        with pytest.raises(MsbwtError):
            b.locate_kmer(np.array([LETTER.index(c) for c in longest[-k:]], dtype=np.uint8), 3)


# ---- 7. rows past 2^32 ----

def long_runs():
    """70 runs of 2^25 .. 2^27 symbols with 200 short ones among them: about 5.5e9 rows, a few hundred bytes of RLE"""
    rng = np.random.default_rng(32)
    lens = rng.integers(1 << 25, 1 << 27, size=70)
    at = np.sort(rng.integers(0, 71, size=200))
    lens = np.insert(lens, at, rng.integers(1, 300, size=200))
    syms = np.zeros(lens.size, dtype=np.int64)
    syms[0] = 5
    for i in range(1, lens.size):  # no neighbours alike; '$' in short runs only, so that most walks go on for a while
        syms[i] = (syms[i - 1] + rng.integers(1, 6)) % 6
        while syms[i] == 0 and lens[i] >= 1 << 25:
            syms[i] = (syms[i - 1] + rng.integers(1, 6)) % 6
    return syms, lens


@pytest.mark.parametrize("blocks", ["planes", "runs"])
def test_rows_past_32_bits(blocks, monkeypatch):
    import torch
    syms, lens = long_runs()
    index = W.Runs(syms, lens)
    assert index.T > (1 << 32) + (1 << 24) and index.reads > 0
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device("cuda", 0))
    if free < 12e9:
        pytest.skip("needs 12 GB of free HBM")
    b = msbwt.RleBWT(device=0)
    b.set_block_format(blocks)
    b.set_pair_index(0)
    b.set_sparse_table(0)
    b.load_vector(runs_to_bytes(syms, lens))
    assert b.get_total_size() == index.T and b.get_block_format() == blocks
    print("%s blocks of %d rows: device_bytes() = %.2f GB" % (blocks, index.T, b.device_bytes() / 1e9))
    rng = np.random.default_rng(4)
    edge = np.int64(1) << 32
    rows = np.concatenate([edge + np.arange(-40, 40), index.starts, index.ends - 1, rng.integers(0, index.T, size=4000), rng.integers(edge, index.T, size=2000),
                           np.arange(index.reads - 20, index.reads + 20), [index.T - 1, 0]]).astype(U64)
    want = W.expected_arrays(index, rows, 50, fill=SENTINEL)
    # walks start on both sides of 2^32 and cross it in both directions
    below, above = rows < U64(edge), rows >= U64(edge)
    step1 = index.step_many(rows.astype(np.int64))[1]
    assert (step1[below] >= edge).any() and (step1[above] < edge).any() and (want[2] == W.DOLLAR).any() and (want[2] == W.MAX_STEPS).any()
    rc, got = raw_walk(b, rows, 50)
    assert rc == 0
    check(got, want, blocks)
    got = b.walk_rows(torch.from_numpy(rows.view(np.int64)).cuda(), 50)
    b.device_status(torch.cuda.current_stream().cuda_stream)
    check(got, W.expected_arrays(index, rows, 50), (blocks, "device"))
    rc, got = raw_walk(b, np.array([index.T, index.T - 1], dtype=U64), 2)
    assert rc == _lib.ERR_INVALID_RANGE and got[2].tolist()[0] == W.BAD_ROW
