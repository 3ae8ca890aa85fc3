"""The guards of the k-mer walk calls (csrc/walk_call.hpp, csrc/spectrum.cpp, csrc/graph_calls.cpp) -- the spectra, the dumps in both forms and the degree table of the plain,
canonical, by-source and graph families -- as their callers see them: the return code AND the whole text msbwt_rle_last_error gives,
for a k out of range, limits the wrong way round, a histogram too short, a NULL out_n and a capacity between 0 and n; the order the
checks fire in (no index before any argument, no sources before k, k before the limits); and the scratch a plain or a canonical call
allocates against its plan.  The texts are recorded behaviour: they were written down from the library as it was before the calls
were given one frame, and hold for it as they do for this one.

One index throughout: the three ragged read sets of test_gpu_source_spectrum.three_sets() merged (a few thousand rows), k = 8.  Run
with `pytest -m gpu`."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_reads_build import naive_rle
from test_gpu_source_spectrum import three_sets

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
U64 = np.uint64
NO_LIMIT = (1 << 64) - 1
K = 8
INVALID, NOT_LOADED = _lib.ERR_INVALID_ARG, _lib.ERR_NOT_LOADED

_state = {}


def state():
    """(the index with its sources, the same index without, an empty handle, the stream), made once"""
    if not _state:
        import torch
        from oracle import oracle
        rles = [naive_rle(oracle, s) for s in three_sets()]
        with_sources, without = msbwt.RleBWT(device=0), msbwt.RleBWT(device=0)
        with_sources.load_merged_many(rles, keep_sources=True)
        without.load_merged_many(rles, keep_sources=False)
        assert with_sources.source_count() == 3 and without.source_count() == 0
        _state.update(b=with_sources, plain=without, empty=msbwt.RleBWT(device=0), stream=torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    return _state


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def said(b):
    return _lib.lib().msbwt_rle_last_error(b._h).decode()


# ---- the calls, each as f(b, k, limits..., outputs..., capacity, out_n) ----

def spectrum_call(name):
    """(b, k, hist, bins) -> rc of msbwt_rle_<name>"""
    def call(b, k, hist, bins):
        fn = getattr(_lib.lib(), "msbwt_rle_" + name)
        extra = (None, None, None) if name == "kmer_spectrum_by_source" else (None, None)
        return fn(b._h, k, _ptr(hist), bins, *extra)
    return call


def dump_call(family, device):
    """(b, k, lo, hi, outs, capacity, out_n) -> rc; lo/hi: min_count/max_count, the totals of the by-source call, min_count/min_edge
    of the graph; outs: the pointers (host arrays' or device addresses) of the family's columns"""
    lib = _lib.lib()
    fn = getattr(lib, "msbwt_rle_enumerate_" + family + ("_device" if device else ""))

    def call(b, k, lo, hi, outs, capacity, out_n, lows=None, highs=None):
        tail = (state()["stream"],) if device else ()
        if family == "kmers":
            return fn(b._h, k, lo, hi, 1, *outs, capacity, out_n, *tail)
        if family == "kmers_by_source":
            return fn(b._h, k, _ptr(lows), _ptr(highs), lo, hi, 1, *outs, capacity, out_n, *tail)
        return fn(b._h, k, lo, hi, *outs, capacity, out_n, *tail)  # canonical_kmers, kmer_graph
    return call


SPECTRA = [("kmer_spectrum", "a histogram"), ("canonical_kmer_spectrum", "a histogram"), ("kmer_spectrum_by_source", "histograms")]
FAMILIES = [("kmers", 3, "k-mers"), ("canonical_kmers", 3, "classes"), ("kmers_by_source", 3, "k-mers"), ("kmer_graph", 4, "k-mers")]
DUMPS = [(family, columns, things, device) for family, columns, things in FAMILIES for device in (False, True)]


def degrees(b, k, min_count, min_edge, table=None, nodes=None, edges=None):
    return _lib.lib().msbwt_rle_kmer_graph_degrees(b._h, k, min_count, min_edge, _ptr(table), nodes, edges)


# ---- 1. k out of range ----

@pytest.mark.parametrize("k", [0, 33])
def test_k_out_of_range(k):
    b = state()["b"]
    hist, n = np.zeros(8, dtype=U64), C.c_uint64(7)
    for name, _ in SPECTRA:
        assert spectrum_call(name)(b, k, hist, 8) == INVALID and said(b) == name + " needs 1 <= k <= 32"
    for family, columns, _, device in DUMPS:
        # (k is looked at before the limits and before the pointers)
        assert dump_call(family, device)(b, k, 3, 2, (None,) * columns, 5, None) == INVALID
        assert said(b) == "enumerate_" + family + " needs 1 <= k <= 32", (family, device)
    assert degrees(b, k, 3, 2, nodes=C.byref(n)) == INVALID and said(b) == "kmer_graph_degrees needs 1 <= k <= 32" and n.value == 7


# ---- 2. limits the wrong way round ----

def test_limits_the_wrong_way_round():
    b = state()["b"]
    n = C.c_uint64(7)
    for family, columns, _, device in DUMPS:
        call, none, name = dump_call(family, device), (None,) * columns, "enumerate_" + family
        # (the limits are looked at before the pointers)
        assert call(b, K, 3, 2, none, 5, None) == INVALID, (family, device)
        want = {"kmers": ": min_count > max_count", "canonical_kmers": ": min_count > max_count", "kmers_by_source": ": min_total > max_total",
                "kmer_graph": ": min_edge is below the node threshold (0 = the node threshold)"}[family]
        assert said(b) == name + want, (family, device)
        if family != "kmer_graph":
            assert call(b, K, 3, 0, none, 0, C.byref(n)) == 0  # 0 = no upper limit
        if family == "kmers_by_source":
            lows, highs = np.array([0, 2, 0], dtype=U64), np.array([NO_LIMIT, 1, NO_LIMIT], dtype=U64)
            # (the per-source pairs before the totals)
            assert call(b, K, 3, 2, none, 0, C.byref(n), lows, highs) == INVALID and said(b) == name + ": min_counts[1] > max_counts[1]"
            assert call(b, K, 1, 0, none, 0, C.byref(n), np.array([0, 0, 5], dtype=U64), np.array([9, 9, 4], dtype=U64)) == INVALID
            assert said(b) == name + ": min_counts[2] > max_counts[2]"
    assert degrees(b, K, 3, 2, nodes=C.byref(n)) == INVALID
    assert said(b) == "kmer_graph_degrees: min_edge is below the node threshold (0 = the node threshold)"
    assert degrees(b, K, 0, 0) == 0 and degrees(b, K, 2, 2, nodes=C.byref(n)) == 0  # NULL table, nodes and edges are all tolerated


# ---- 3. fewer than 2 bins ----

def test_fewer_than_two_bins():
    b = state()["b"]
    hist = np.full(8, 7, dtype=U64)
    for name, what in SPECTRA:
        for bins in (0, 1):
            assert spectrum_call(name)(b, K, hist, bins) == INVALID and said(b) == "%s needs %s of at least 2 bins" % (name, what), (name, bins)
        assert spectrum_call(name)(b, K, None, 8) == INVALID and said(b) == "%s needs %s of at least 2 bins" % (name, what), name
        assert spectrum_call(name)(b, 33, None, 1) == INVALID and said(b) == name + " needs 1 <= k <= 32"  # k first
    assert (hist == 7).all()


# ---- 4. NULL out_n, and a capacity without the k-mer column ----

def test_null_pointers():
    b = state()["b"]
    n = C.c_uint64(7)
    for family, columns, _, device in DUMPS:
        call, none = dump_call(family, device), (None,) * columns
        want = "null pointer" if family == "kmer_graph" or not device else "null device pointer"
        assert call(b, K, 1, 0, none, 0, None) == INVALID and said(b) == want, (family, device)
        if family != "kmer_graph":  # (the graph's columns are all optional)
            assert call(b, K, 1, 0, none, 5, C.byref(n)) == INVALID and said(b) == want and n.value == 7, (family, device)


# ---- 5. 0 < capacity < n ----

def test_capacity_between_zero_and_n():
    import torch
    dev = torch.device("cuda:0")
    b, stream = state()["b"], state()["stream"]
    S = 3
    for family, columns, things, device in DUMPS:
        call, n = dump_call(family, device), C.c_uint64(0)
        assert call(b, K, 1, 0, (None,) * columns, 0, C.byref(n)) == 0
        full = n.value
        assert full > 32
        widths = [1, S, 1] if family == "kmers_by_source" else [1] * columns
        for capacity in (1, full - 1):
            if device:
                bufs = [torch.full((full * w,), -7, dtype=torch.int64, device=dev) for w in widths]
                outs = tuple(t.data_ptr() for t in bufs)
            else:
                bufs = [np.full(full * w, 7, dtype=U64) for w in widths]
                outs = tuple(_ptr(a) for a in bufs)
            n.value = 0
            assert call(b, K, 1, 0, outs, capacity, C.byref(n)) == INVALID, (family, device, capacity)
            assert said(b) == "enumerate_%s: capacity %d is less than the n = %d %s that qualify" % (family, capacity, full, things), (family, device)
            assert n.value == full
            assert all(bool((t == -7).all()) for t in bufs) if device else all((a == 7).all() for a in bufs)  # nothing written
        n.value = 0
        assert call(b, K, 1, 0, outs, full, C.byref(n)) == 0 and n.value == full  # and exactly n is enough
    b.device_status(stream)


# ---- 6. the order of the checks: no index, then no sources, then the arguments ----

def test_no_index_comes_first():
    e = state()["empty"]
    hist = np.zeros(8, dtype=U64)
    for name, _ in SPECTRA:
        assert spectrum_call(name)(e, 0, hist, 1) == NOT_LOADED and said(e) == "no BWT loaded", name
    for family, columns, _, device in DUMPS:
        assert dump_call(family, device)(e, 0, 3, 2, (None,) * columns, 5, None) == NOT_LOADED and said(e) == "no BWT loaded", (family, device)
    assert degrees(e, 0, 3, 2) == NOT_LOADED and said(e) == "no BWT loaded"


def test_no_sources_attached():
    p = state()["plain"]
    hist, n = np.zeros(8, dtype=U64), C.c_uint64(7)
    for k, bins in ((K, 8), (0, 1)):  # (before k and the bins)
        assert spectrum_call("kmer_spectrum_by_source")(p, k, hist, bins) == NOT_LOADED and said(p) == "no sources attached"
    for device in (False, True):
        call = dump_call("kmers_by_source", device)
        assert call(p, K, 1, 0, (None,) * 3, 0, C.byref(n)) == NOT_LOADED and said(p) == "no sources attached" and n.value == 7
        assert call(p, 0, 3, 2, (None,) * 3, 5, None) == NOT_LOADED and said(p) == "no sources attached"
    assert spectrum_call("kmer_spectrum")(p, K, hist, 8) == 0  # the other families do not ask for sources
    assert dump_call("kmers", False)(p, K, 1, 0, (None,) * 3, 0, C.byref(n)) == 0 and n.value > 32


# ---- 7. a refused call leaves the record of the last walk as it was ----

def test_a_refused_call_leaves_the_last_walk_s_record():
    b = state()["b"]
    b.kmer_spectrum(K, 64)
    info, scratch = b.spectrum_info(), b.spectrum_scratch_bytes()
    assert info["k"] == K and scratch > 0
    n = C.c_uint64(0)
    assert dump_call("kmers", False)(b, 33, 1, 0, (None,) * 3, 0, C.byref(n)) == INVALID
    assert dump_call("canonical_kmers", False)(b, K, 3, 2, (None,) * 3, 0, C.byref(n)) == INVALID
    assert degrees(b, K, 3, 2) == INVALID
    after = b.spectrum_info()
    assert after["k"] == K and np.array_equal(after["nodes"], info["nodes"]) and after["ms"] == info["ms"] and b.spectrum_scratch_bytes() == scratch


# ---- 8. the plan is what a plain and a canonical call allocate ----

def test_the_plan_is_what_a_plain_and_a_canonical_call_allocate():
    """msbwt_spectrum_plan and msbwt_canonical_plan against msbwt_rle_spectrum_scratch_bytes, as the by-source and the graph tests
    hold theirs.  rows + 1024 < 2^20, so the automatic frontier is the index's whatever is free; 64 bins and more than 32 records, so
    every allocation is above the 256 bytes one is rounded up to.  A canonical call takes 256 bytes above its plan: the words of its
    totals, an allocation of their own that msbwt_canonical_plan leaves out."""
    import torch
    dev = torch.device("cuda:0")
    b, stream = state()["b"], state()["stream"]
    free, total = torch.cuda.mem_get_info(0)[0], b.get_total_size()
    assert total + 1024 < 2 ** 20
    plan = lambda records=0, srt=False: msbwt.spectrum_plan(total, free, records, srt)
    cplan = lambda records=0: msbwt.canonical_plan(total, free, records)
    assert plan() == msbwt.spectrum_plan(total, 10 ** 9) and cplan() == msbwt.canonical_plan(total, 10 ** 9)
    took = b.spectrum_scratch_bytes
    for bins in (32, 64, 256):
        b.kmer_spectrum(K, bins)
        assert took() == plan() + 8 * bins, bins
        b.canonical_kmer_spectrum(K, bins)
        assert took() == cplan() + 256 + 8 * bins, bins
    # plain
    lib, got = _lib.lib(), C.c_uint64(0)
    for srt in (True, False):
        n = b.enumerate_kmers_device(K, None, None, None, 0, sorted=srt, stream=stream)
        assert n > 32 and took() == plan(), srt  # counting marks nothing
        bufs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
        assert b.enumerate_kmers_device(K, *[t.data_ptr() for t in bufs], n, sorted=srt, stream=stream) == n
        assert took() == plan(0, srt), srt  # device form: no records staged
        b.enumerate_kmers(K, sorted=srt, ranges=True)
        assert took() == plan(n, srt), srt  # host form: word, count and l per record
        assert plan(n, srt) - plan(0, srt) == 24 * n
        b.enumerate_kmers(K, sorted=srt)
        assert took() == plan(n, srt) - 8 * n, srt  # ... without l
        w, l = np.empty(n, dtype=U64), np.empty(n, dtype=U64)
        assert lib.msbwt_rle_enumerate_kmers(b._h, K, 1, 0, int(srt), _ptr(w), None, _ptr(l), n, C.byref(got)) == 0
        assert took() == plan(n, srt) - 8 * n, srt  # ... without the counts
        assert lib.msbwt_rle_enumerate_kmers(b._h, K, 1, 0, int(srt), _ptr(w), None, None, n, C.byref(got)) == 0
        assert took() == plan(n, srt) - 16 * n, srt
    assert plan(0, True) > plan(0, False)
    # canonical
    n = b.enumerate_canonical_kmers_device(K, None, None, None, 0, stream=stream)
    assert n > 32 and took() == cplan() + 256
    bufs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
    assert b.enumerate_canonical_kmers_device(K, *[t.data_ptr() for t in bufs], n, stream=stream) == n
    assert took() == cplan() + 256
    b.enumerate_canonical_kmers(K, strands=True)
    assert took() == cplan(n) + 256 and cplan(n) - cplan() == 24 * n
    w, o = np.empty(n, dtype=U64), np.empty(n, dtype=U64)
    assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, K, 1, 0, _ptr(w), None, _ptr(o), n, C.byref(got)) == 0
    assert took() == cplan(n) + 256 - 8 * n
    assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, K, 1, 0, _ptr(w), None, None, n, C.byref(got)) == 0
    assert took() == cplan(n) + 256 - 16 * n
    b.device_status(stream)
