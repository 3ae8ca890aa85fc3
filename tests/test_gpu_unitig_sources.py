"""Unitigs by source (csrc/unitig_sources.hip and its driver in csrc/unitig_calls.cpp): the U x S matrix
msbwt_rle_enumerate_unitig_graph_by_source and msbwt_rle_enumerate_canonical_unitig_graph_by_source return behind the link table.

Every expected matrix comes from tests/colour_oracle.py -- Counters of the k-windows per source over the unitigs of the string oracles,
numpy censuses per source on the large sets -- which tests/test_colour_oracle.py checks on the CPU.  The seven columns of the graph
call are compared byte for byte with what msbwt_rle_enumerate_[canonical_]unitig_graph returns on the same handle, in both forms.

1. Hand-made and ragged sets at every k of the unitig tests, S in (1, 2, 3, 4, 5, 9, 32), four threshold pairs, empty inputs included.
2. Identities that need no oracle: row sums, column sums against kmer_spectrum_by_source, relabelled sources, one source.
3. The two counting paths: ranges 239, 240, 241 and 300 rows wide over three sources, some across a multiple of 1024 rows.
4. Canonical particulars, a chain over several tiles, a circle, a self-loop.
5. The scale set of tests/test_gpu_graph_scale.py dealt to 4 sources, under both frontiers: several chunks, several trips.
6. Every index form and the minimum frontier; capacities, NULL buffers, tails, scratch against the plans; the guards.
7. Past 2^32 rows; the example program.
Run with `pytest -m gpu`."""
import bisect
import ctypes as C
import importlib
import os
import subprocess
import time

import numpy as np
import pytest

import colour_oracle as CO
import graph_oracle as G
from conftest import ROOT
from test_gpu_canonical_unitigs import flip_every_second, rc
from test_gpu_graph_scale import EDGE_CHUNK, FRONTIERS, TRIP, scale_set, scale_want
from test_gpu_kmer_graph import FORMS
from test_gpu_merge_many import EMPTY, homopolymer_rle, ragged_collection
from test_gpu_reads_build import naive_rle, ragged_set
from test_gpu_source_spectrum import merged
from test_gpu_spectrum import loaded
from test_gpu_unitigs import chain
from test_graph_oracle import HAND_MADE
from test_unitigs_abi import _link_flags

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
NAMES = G.NAMES + ("link_offsets", "link_targets")
KS = (1, 2, 3, 4, 15, 16, 17, 30, 31)
PAIRS = ((1, 0), (2, 0), (2, 3), (10 ** 6, 0))  # the last one leaves no node
SOURCES = (1, 2, 3, 4, 5, 9, 32)  # each side of four sources a dword and of the 8-lane striding, and the maximum


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def merged_texts(orc, sets):
    return merged([naive_rle(orc, s) if s else EMPTY for s in sets])


def device_call(b, k, pair, canonical, sizes):
    """the _device form into buffers of exactly the sizes the host form reported -> the eight columns"""
    import torch
    dev = torch.device("cuda:0")
    words = ("offsets", "count_sums", "link_offsets", "link_targets", "source_sums")
    bufs = {x: torch.full((n,), 7, dtype=torch.int64 if x in words else torch.uint8, device=dev) for x, n in sizes.items()}
    fn = b.enumerate_canonical_unitig_graph_by_source_device if canonical else b.enumerate_unitig_graph_by_source_device
    ptrs = [bufs[x].data_ptr() if sizes[x] else None for x in NAMES + ("source_sums",)]
    U, S, L = fn(k, *ptrs, sizes["count_sums"], sizes["symbols"], sizes["link_targets"], min_count=pair[0], min_edge=pair[1] or None,
                 stream=torch.cuda.current_stream(dev).cuda_stream)
    b.device_status(torch.cuda.current_stream(dev).cuda_stream)
    assert (U, S, L) == (sizes["count_sums"], sizes["symbols"], sizes["link_targets"])
    return [bufs[x].cpu().numpy().view(U64) if x in words else bufs[x].cpu().numpy() for x in NAMES + ("source_sums",)]


def check(b, k, pair, canonical, count_sums, matrix, where, device=True):
    """the new call against the oracle's count sums and matrix, its seven columns against the graph call on the same handle"""
    n_sources = b.source_count()
    got = b.enumerate_unitig_graph_by_source(k, min_count=pair[0], min_edge=pair[1] or None, canonical=canonical)
    report = b.canonical_unitig_info if canonical else b.unitig_info
    info = report()
    graph = b.enumerate_unitig_graph(k, min_count=pair[0], min_edge=pair[1] or None, canonical=canonical)
    assert report() == info, where
    assert len(got) == 8
    for name, g, o in zip(NAMES, got, graph):
        assert g.dtype == o.dtype and g.tobytes() == o.tobytes(), (where, name)
    m = got[7]
    assert m.dtype == U64 and m.shape == (len(got[2]), n_sources) == matrix.shape, (where, m.shape, matrix.shape)
    assert np.array_equal(got[2], count_sums), where
    bad = np.argwhere(m != matrix)
    assert bad.size == 0, (where, bad[:5], m[tuple(bad[:5].T)], matrix[tuple(bad[:5].T)])
    assert np.array_equal(m.sum(axis=1), got[2]), where
    if device and len(got[2]):
        sizes = {x: len(g) for x, g in zip(NAMES, got)}
        sizes["source_sums"] = m.size
        for name, g, d in zip(NAMES + ("source_sums",), got, device_call(b, k, pair, canonical, sizes)):
            assert d.tobytes() == g.tobytes(), (where, name, "device")
    return got


def check_texts(b, sets, k, pair, canonical, where):
    unitigs, matrix = CO.unitigs_by_source(sets, k, pair[0], pair[1], canonical)
    return check(b, k, pair, canonical, unitigs["count_sums"], matrix, where)


# ---- 1. hand-made and ragged sets ----

def collection(S, seed):
    """S read sets: ragged, with reads repeated across them, an empty set and a set of one empty read where there is room"""
    if S >= 3:
        return ragged_collection(S, seed)
    return CO.deal(ragged_set(seed) + ["GGACGTCCTAGCATGCTAGG"] * 2, S)


@pytest.mark.parametrize("S", SOURCES)
def test_ragged_collections(orc, S):
    sets = collection(S, 1)
    if S >= 3:
        assert [""] in sets and ([] in sets or S == 4)  # (of 4 sets the empty one and the one of an empty read are the same set)
    b = merged_texts(orc, sets)
    rows = 0
    for k in KS + (32,):
        for pair in PAIRS:
            for canonical in (False, True) if k <= 31 else (False,):
                got = check_texts(b, sets, k, pair, canonical, (S, k, pair, canonical))
                rows += len(got[2])
                assert pair[0] < 10 ** 6 or len(got[2]) == 0
    assert rows > 100


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_sets(orc, name):
    reads = HAND_MADE[name]
    splits = {"dealt to 2": CO.deal(reads * 2, 2), "three, one of mirrors only": [list(reads), [rc(r) for r in reads], []],
              "flipped, dealt to 3": CO.deal(flip_every_second(reads * 3), 3)}
    for split, sets in splits.items():
        b = merged_texts(orc, sets)
        for k in (1, 2, 3, 4, 5, 6):
            for pair in PAIRS[:3]:
                for canonical in (False, True):
                    check_texts(b, sets, k, pair, canonical, (name, split, k, pair, canonical))


def test_an_index_without_a_node(orc):
    b = merged_texts(orc, [["", "NN"], []])
    for canonical in (False, True):
        got = b.enumerate_unitig_graph_by_source(5, canonical=canonical)
        assert [len(a) for a in got] == [0, 1, 0, 0, 0, 1, 0, 0] and got[7].shape == (0, 2) and got[5].tolist() == [0]
        fn = _lib.lib().msbwt_rle_enumerate_canonical_unitig_graph_by_source if canonical else _lib.lib().msbwt_rle_enumerate_unitig_graph_by_source
        u, s, n = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        side, matrix = np.full(3, 7, dtype=U64), np.full(4, 7, dtype=U64)
        assert fn(b._h, 5, 1, 0, None, None, None, None, None, side.ctypes.data_as(C.c_void_p), None, matrix.ctypes.data_as(C.c_void_p), 4, 4, 4,
                  C.byref(u), C.byref(s), C.byref(n)) == 0
        assert (u.value, s.value, n.value) == (0, 0, 0) and side.tolist() == [0, 7, 7] and (matrix == 7).all()


# ---- 2. identities that need no oracle ----

def test_identities(orc):
    sets = collection(5, 3)
    rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
    b = merged(rles)
    builder = msbwt.RleBWT(device=0)
    rle, sources = builder.merge_many(rles, return_sources=True)
    order = np.array([3, 0, 4, 1, 2], dtype=np.uint8)  # source s becomes order[s]
    relabelled = loaded(rle)
    relabelled.set_sources(order[sources], 5)
    one = loaded(rle)
    one.set_sources(np.zeros_like(sources), 1)
    for k in (1, 4, 16, 31):
        for canonical in (False, True):
            got = b.enumerate_unitig_graph_by_source(k, canonical=canonical)
            m = got[7]
            assert len(m) and np.array_equal(m.sum(axis=1), got[2])
            if not canonical:
                assert np.array_equal(m.sum(axis=0), b.kmer_spectrum_by_source(k)[3])
            again = relabelled.enumerate_unitig_graph_by_source(k, canonical=canonical)
            assert all(a.tobytes() == g.tobytes() for a, g in zip(again[:7], got[:7]))
            assert np.array_equal(again[7][:, order], m)
            single = one.enumerate_unitig_graph_by_source(k, canonical=canonical)
            assert single[7].shape == (len(m), 1) and np.array_equal(single[7][:, 0], got[2])


# ---- 3. the two counting paths ----

def test_both_counting_paths_and_a_checkpoint_border():
    narrow, block = msbwt.source_narrow_rows(), msbwt.source_block_rows()
    assert (narrow, block) == (240, 1024)
    rng = np.random.default_rng(77)
    text = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, size=n))
    k, copies = 12, (239, 240, 241, 300)
    repeated = [text(24) for _ in copies]
    sets = [[], [], []]
    for read, c in zip(repeated, copies):  # unevenly: 100 copies, 50 copies, the rest
        sets[0] += [read] * 100
        sets[1] += [read] * 50
        sets[2] += [read] * (c - 150)
    for i in range(600):
        sets[i % 3].append(text(30))
    # the rows of the merged index are the suffixes of every read and its '$' in order: the range of q from the strings alone
    suffixes = sorted((r + "$")[i:] for s in sets for r in s for i in range(len(r) + 1))
    widths, crossing = set(), {"narrow": 0, "wide": 0}
    for read in repeated:
        for i in range(len(read) - k + 1):
            q = read[i:i + k]
            l, h = bisect.bisect_left(suffixes, q), bisect.bisect_left(suffixes, q + "~")
            widths.add(h - l)
            if l // block != (h - 1) // block:
                crossing["narrow" if h - l <= narrow else "wide"] += 1
    assert widths == set(copies) and crossing["narrow"] >= 1 and crossing["wide"] >= 1, (widths, crossing)
    builder = msbwt.RleBWT(device=0)
    b = merged([builder.build_from_reads(s, ascii=True) for s in sets])
    assert b.get_total_size() == len(suffixes)
    for canonical in (False, True):
        got = check_texts(b, sets, k, (1, 0), canonical, ("counting paths", canonical))
        assert {239, 240, 241, 300} <= set((got[7].sum(axis=1) // U64(13)).tolist())  # the repeated reads: one unitig of 13 nodes each


# ---- 4. canonical particulars and shapes ----

def test_canonical_particulars(orc):
    # the palindromic node mid-path counts once; GGAC and GTCC are one class
    sets = [["GGACGTCC"], ["GGACGTCC", "ACGT"]]
    got = check_texts(merged_texts(orc, sets), sets, 4, (1, 0), True, "palindrome")
    assert got[7].tolist() == [[1, 2], [4, 4]]
    # a source on the reverse strand only lands in the emitted unitig's row, whose sequence is the mirror of what source 0 spells
    sets = [["TTACG"], [rc("TTACG")], [rc("TTACG")] * 2]
    b = merged_texts(orc, sets)
    got = check_texts(b, sets, 5, (1, 0), True, "mirror only")
    assert b.enumerate_unitig_graph_by_source(5, canonical=True, text=True)[0] == ["CGTAA"] and got[7].tolist() == [[1, 1, 2]]
    # every count from skipped slots: the reads spell TTACG.. only, the emitted unitig is its mirror
    sets = [["TTACGG"], ["TTACGG"] * 2]
    got = check_texts(merged_texts(orc, sets), sets, 5, (1, 0), True, "skipped slots")
    assert got[7].tolist() == [[2, 4]]


@pytest.mark.parametrize("circular", [False, True], ids=["chain", "circle"])
def test_one_long_unitig(circular):
    reads, _ = chain(circular)
    sets = CO.deal(reads, 3)
    builder = msbwt.RleBWT(device=0)
    b = merged([builder.build_from_reads(s, ascii=True) for s in sets])
    for k in (21, 31):
        for canonical in (False, True):
            unitigs, matrix = CO.unitigs_by_source(sets, k, canonical=canonical)
            assert len(matrix) == 1 and unitigs["info"]["longest"] > (2048 if circular else 4 * 2048)
            got = check(b, k, (1, 0), canonical, unitigs["count_sums"], matrix, (circular, k, canonical))
            assert got[4].tolist() == [1 if circular else 0]


# ---- 5. multi-trip sizes ----

_scale = {}


def scale_sources():
    """(the scale set dealt to 4 sources as code arrays, a handle of their merge), made once"""
    if not _scale:
        sets = CO.deal(scale_set(), 4)
        t0 = time.perf_counter()
        builder = msbwt.RleBWT(device=0)
        rles = []
        for s in sets:
            offsets = np.zeros(len(s) + 1, dtype=U64)
            np.cumsum([r.size for r in s], out=offsets[1:])
            rles.append(builder.build_from_reads((np.concatenate(s), offsets)))
        b = merged(rles)
        print("scale set in 4 sources: built and merged in %.2f s" % (time.perf_counter() - t0))
        _scale.update(sets=sets, b=b)
    return _scale["sets"], _scale["b"]


@pytest.mark.parametrize("frontier", sorted(FRONTIERS))
def test_the_scale_set_in_four_sources(frontier):
    k, pair = 21, (1, 0)
    sets, b = scale_sources()
    b.set_spectrum_frontier(FRONTIERS[frontier])
    try:
        for canonical in (False, True):
            want = scale_want("canonical" if canonical else "plain", k, pair)
            assert want["info"]["nodes" if not canonical else "classes"] > TRIP and (not canonical or want["slots"] > EDGE_CHUNK)
            t0 = time.perf_counter()
            matrix = CO.source_sums_of_codes(sets, k, want["symbols"], want["offsets"], canonical)
            t1 = time.perf_counter()
            check(b, k, pair, canonical, want["count_sums"], matrix, (frontier, canonical), device=not canonical)
            print("scale set, %s, %s: %d unitigs, oracle %.1f s, calls %.2f s"
                  % (frontier, "canonical" if canonical else "plain", len(matrix), t1 - t0, time.perf_counter() - t1))
    finally:
        b.set_spectrum_frontier(0)


# ---- 6. index forms, the contract, the guards ----

def contract_set(orc):
    if "contract" not in _scale:
        sets = collection(4, 5)
        rles = [naive_rle(orc, s) if s else EMPTY for s in sets]
        rle, sources = msbwt.RleBWT(device=0).merge_many(rles, return_sources=True)
        _scale["contract"] = (sets, rle, sources)
    return _scale["contract"]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_index_form_and_the_minimum_frontier(orc, form):
    sets, rle, sources = contract_set(orc)
    b = loaded(rle, **FORMS[form])
    b.set_sources(sources, 4)
    for frontier in (0, _lib.SPECTRUM_MIN_FRONTIER):
        b.set_spectrum_frontier(frontier)
        for k in (4, 17):
            for canonical in (False, True):
                check_texts(b, sets, k, (1, 0), canonical, (form, frontier, k, canonical))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
def test_capacities_null_buffers_and_scratch(orc, canonical):
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    sets, rle, sources = contract_set(orc)
    k, min_count, n_sources = 6, 1, 4
    unitigs, matrix = CO.unitigs_by_source(sets, k, min_count, 0, canonical)
    b = loaded(rle)
    b.set_sources(sources, n_sources)
    want = dict(zip(NAMES, b.enumerate_unitig_graph(k, min_count=min_count, canonical=canonical)))
    want["source_sums"] = matrix.reshape(-1)
    ALL = NAMES + ("source_sums",)
    n, U, S, Ln = unitigs["info"]["classes" if canonical else "nodes"], len(want["count_sums"]), len(want["symbols"]), len(want["link_targets"])
    assert U > 20 and Ln > 20 and np.array_equal(want["count_sums"], unitigs["count_sums"])
    lib, got_u, got_s, got_l = _lib.lib(), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    host_fn = lib.msbwt_rle_enumerate_canonical_unitig_graph_by_source if canonical else lib.msbwt_rle_enumerate_unitig_graph_by_source
    device = b.enumerate_canonical_unitig_graph_by_source_device if canonical else b.enumerate_unitig_graph_by_source_device
    total, before, free = b.get_total_size(), b.device_bytes(), torch.cuda.mem_get_info(0)[0]
    plan = lambda *a: msbwt.unitig_graph_by_source_plan(total, free, *a, n_sources=n_sources, canonical=canonical)
    graph_plan = lambda *a: msbwt.unitig_graph_plan(total, free, *a, canonical=canonical)
    pad = lambda x: (x + 255) // 256 * 256
    ranges = pad(8 * (2 * min(2 * n, EDGE_CHUNK) if canonical else n))
    assert plan(n) == graph_plan(n) and plan(n, U, S, Ln) == graph_plan(n, U, S, Ln) + ranges + pad(8 * U * n_sources)
    sizes = dict({x: len(want[x]) for x in NAMES}, source_sums=U * n_sources)
    staged = {"symbols": 8 * ((S + 7) // 8), "offsets": 0, "count_sums": 8 * U, "ends": 8 * ((U + 7) // 8), "flags": 8 * ((U + 7) // 8), "link_offsets": 0,
              "link_targets": 8 * Ln, "source_sums": ranges + pad(8 * U * n_sources)}

    def host(cap_u, cap_s, cap_l, skip=()):
        bufs = {x: np.full(sizes[x] + 3, 7, dtype=want[x].dtype) for x in ALL}
        args = [_ptr(bufs[x]) if x not in skip else None for x in ALL]
        return host_fn(b._h, k, min_count, 0, *args, cap_u, cap_s, cap_l, C.byref(got_u), C.byref(got_s), C.byref(got_l)), bufs

    # the counting call allocates what the graph call's does; a capacity too small writes nothing, the matrix included
    rc_, bufs = host(0, 0, 0)
    assert rc_ == 0 and (got_u.value, got_s.value, got_l.value) == (U, S, Ln) and all((a == 7).all() for a in bufs.values())
    assert b.spectrum_scratch_bytes() == plan(n) == graph_plan(n)
    for caps in ((U - 1, S, Ln), (U, S - 1, Ln), (U, S, Ln - 1), (1, 1, 1), (0, S, Ln), (0, 0, Ln)):
        got_u.value = got_s.value = got_l.value = 0
        rc_, bufs = host(*caps)
        message = lib.msbwt_rle_last_error(b._h)
        assert rc_ == _lib.ERR_INVALID_ARG and (got_u.value, got_s.value, got_l.value) == (U, S, Ln), caps
        assert all(str(x).encode() in message for x in (U, S, Ln)) and all((a == 7).all() for a in bufs.values()), caps
    # every output NULL in turn -- the matrix, and the link table with the matrix wanted --, and all at once; tails stay
    for skip in ((),) + tuple((x,) for x in ALL) + (("link_offsets", "link_targets"), ALL):
        rc_, bufs = host(U + 2, S + 2, Ln + 2, skip)
        assert rc_ == 0 and (got_u.value, got_s.value, got_l.value) == (U, S, Ln), skip
        for x in ALL:
            assert (bufs[x][sizes[x]:] == 7).all() and (np.array_equal(bufs[x][:sizes[x]], want[x]) if x not in skip else (bufs[x] == 7).all()), (skip, x)
        assert b.spectrum_scratch_bytes() == plan(n, U, S, Ln) - sum(staged[x] for x in skip), skip
    # the device form: nothing staged; without the matrix it is the graph call's device form
    assert device(k, *(None,) * 8, 0, 0, 0, min_count=min_count, stream=stream) == (U, S, Ln)
    assert b.spectrum_scratch_bytes() == plan(n)
    words = ("offsets", "count_sums", "link_offsets", "link_targets", "source_sums")
    for skip in ((), ("source_sums",), ("link_offsets", "link_targets")):
        bufs = {x: torch.full((sizes[x] + 9,), 7, dtype=torch.int64 if x in words else torch.uint8, device=dev) for x in ALL}
        ptrs = [None if x in skip else bufs[x].data_ptr() + (0 if x in words else 1) for x in ALL]
        for caps in ((U - 1, S, Ln), (U, S - 1, Ln)):
            with pytest.raises(MsbwtError) as err:
                device(k, *ptrs, *caps, min_count=min_count, stream=stream)
            assert err.value.code == _lib.ERR_INVALID_ARG and (err.value.n, err.value.symbols, err.value.links) == (U, S, Ln)
            assert all(bool((bufs[x] == 7).all()) for x in ALL)
        assert device(k, *ptrs, U + 1, S + 1, Ln + 1, min_count=min_count, stream=stream) == (U, S, Ln)
        b.device_status(stream)
        assert b.spectrum_scratch_bytes() == plan(n, U, S, Ln) - sum(staged.values()) + (0 if "source_sums" in skip else ranges), skip
        for x in ALL:
            got, lead = bufs[x].cpu().numpy(), 0 if x in words else 1
            if x in skip:
                assert (got == 7).all(), (skip, x)
            else:
                assert (got[:lead] == 7).all() and (got[lead + sizes[x]:] == 7).all() and np.array_equal(got[lead:lead + sizes[x]].astype(want[x].dtype), want[x]), (skip, x)
    assert b.device_bytes() == before
    # the guards on a loaded index with sources, then the existing calls as before
    none = (None,) * 8
    for bad_k in (0, 32 if canonical else 33, 1000):
        assert host_fn(b._h, bad_k, 1, 0, *none, 0, 0, 0, C.byref(got_u), C.byref(got_s), C.byref(got_l)) == _lib.ERR_INVALID_ARG
    assert host_fn(b._h, k, 3, 2, *none, 0, 0, 0, C.byref(got_u), C.byref(got_s), C.byref(got_l)) == _lib.ERR_INVALID_ARG
    assert host_fn(b._h, k, 1, 0, *none, 0, 0, 0, None, C.byref(got_s), C.byref(got_l)) == _lib.ERR_INVALID_ARG
    assert host_fn(b._h, k, 0, 0, *none, 0, 0, 0, C.byref(got_u), None, None) == 0
    after = dict(zip(NAMES, b.enumerate_unitig_graph(k, min_count=min_count, canonical=canonical)))
    assert all(after[x].tobytes() == want[x].tobytes() for x in NAMES) and b.spectrum_scratch_bytes() == graph_plan(n, U, S, Ln)
    old = (b.enumerate_canonical_unitigs if canonical else b.enumerate_unitigs)(k, min_count=min_count)
    assert all(np.array_equal(o, want[x] & 1 if x == "flags" else want[x]) for x, o in zip(G.NAMES, old))
    # without sources: refused before anything is written, whatever else is wrong with the call
    bare = loaded(rle)
    got_u.value = 77
    for bad_k in (k, 0, 1000):
        rc_, bufs = None, {x: np.full(sizes[x] + 3, 7, dtype=want[x].dtype) for x in ALL}
        assert host_fn(bare._h, bad_k, 3, 2, *[_ptr(bufs[x]) for x in ALL], U, S, Ln, C.byref(got_u), None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_last_error(bare._h) == b"no sources attached" and got_u.value == 77 and all((a == 7).all() for a in bufs.values())
    with pytest.raises(MsbwtError) as err:
        bare.enumerate_unitig_graph_by_source(k, canonical=canonical)
    assert err.value.code == _lib.ERR_NOT_LOADED and "no sources attached" in str(err.value)
    assert all(a.tobytes() == want[x].tobytes() for x, a in zip(NAMES, bare.enumerate_unitig_graph(k, min_count=min_count, canonical=canonical)))


# ---- 7. past 2^32 rows, and the example ----

def test_beyond_2_to_32_rows(tmp_path):
    """The three homopolymer inputs of test_gpu_source_spectrum.test_beyond_2_to_32_rows, 4.41e9 merged rows: the nodes are c^k, each
    a circular unitig of one node, and input i holds n_i,c (length - k + 1) rows of it; T's range lies beyond row 2^32 from k = 28 on.
    The canonical call returns the classes {A^k, T^k} and {C^k, G^k} with the sums of their members' rows."""
    import torch
    started = time.perf_counter()
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
    t1 = time.perf_counter()
    assert b.get_total_size() == total and b.source_count() == 3
    b.set_spectrum_frontier(4096)
    before = b.device_bytes()
    for k in (1, 2, 28, 29):
        per = length - k + 1
        row = {c: [counts.get(c, 0) * per for counts in inputs] for c in "ACGT"}
        seqs, sums, _, flags, _, _, m = b.enumerate_unitig_graph_by_source(k, text=True)
        assert seqs == [c * k for c in "ACGT"] and m.tolist() == [row[c] for c in "ACGT"] and np.array_equal(m.sum(axis=1), sums)
        assert flags.tolist() == ([1] * 4 if k < length else [0] * 4)  # c^(k+1) closes the circle while a read holds it
        seqs, sums, _, flags, _, _, m = b.enumerate_unitig_graph_by_source(k, canonical=True, text=True)
        assert seqs == ["A" * k, "C" * k] and np.array_equal(m.sum(axis=1), sums)
        assert m.tolist() == [[a + t for a, t in zip(row["A"], row["T"])], [c + g for c, g in zip(row["C"], row["G"])]]
    assert b.device_bytes() == before
    print("set-up %.2f s, load %.2f s, the calls %.2f s" % (t0 - started, t1 - t0, time.perf_counter() - t1))


def test_the_example_writes_the_matrix(tmp_path):
    exe = str(tmp_path / "unitigs_by_source")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "unitigs_by_source.c"), "-o", exe] + _link_flags())
    sets = [[r for r in s if r and set(r) <= set("ACGTN")] for s in CO.deal(ragged_set(2) + ragged_set(5), 3)]
    files = []
    for i, s in enumerate(sets):
        files.append(str(tmp_path / ("reads_%d.txt" % i)))
        with open(files[-1], "w") as out:
            out.write("".join(r + "\n" for r in s))
    builder = msbwt.RleBWT(device=0)
    b = merged([builder.build_from_reads(s, ascii=True) for s in sets])
    for canonical in (False, True):
        k, min_count = 7, 1
        r = subprocess.run([exe] + (["--canonical"] if canonical else []) + [str(k), str(min_count)] + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = b.enumerate_unitig_graph_by_source(k, min_count=min_count, canonical=canonical, text=True)
        segments = [line.split("\t") for line in r.stdout.splitlines() if line.startswith("S\t")]
        assert [x[2] for x in segments] == got[0] and len(segments) > 10
        assert [[int(c) for c in x[4][len("sc:Z:"):].split(",")] for x in segments] == got[6].tolist()
        assert all(x[3] == "KC:i:%d" % int(s) and x[4].startswith("sc:Z:") for x, s in zip(segments, got[1]))
