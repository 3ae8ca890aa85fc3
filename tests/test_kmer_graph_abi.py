"""The k-mer graph entry points (include/msbwt_hip.h: msbwt_rle_enumerate_kmer_graph[_device], msbwt_rle_kmer_graph_degrees,
msbwt_kmer_graph_plan) without a GPU: the symbols and their signatures, the guards that answer before a device is touched, the pure
size plan against the formula the header states, the neighbour helpers on hand-made words and bytes, the example, the C++ mirror and
the shim's two copies."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
LIBDIR = os.path.join(ROOT, "rust-msbwt_amd")
NEW = ("msbwt_rle_enumerate_kmer_graph", "msbwt_rle_enumerate_kmer_graph_device", "msbwt_rle_kmer_graph_degrees", "msbwt_kmer_graph_plan")
C4, HUMAN = 1_950_000_000, 90_000_000_000
FREE = 250 * 10 ** 9
U64 = np.uint64


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "void *": C.c_void_p, "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)),
                "uint8_t *": C.c_void_p, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int": C.c_int}
    for name in NEW:
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SIGNATURES[name]
        cret, cparams = decls[name]
        assert ctype_of[shim.norm_c(cret)] == res, name
        assert len(cparams) == len(args), name
        for ct, a in zip(cparams, args):
            want = ctype_of[shim.norm_c(ct)]
            assert a in want if isinstance(want, tuple) else a == want, (name, ct)
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own, after "k-mers by source" and before the scratch report
    assert header.index("msbwt_kmers_by_source_plan(") < header.index("---- the k-mer graph") < header.index("msbwt_rle_enumerate_kmer_graph(")
    assert header.index("msbwt_kmer_graph_plan(uint64_t") < header.index("msbwt_rle_spectrum_scratch_bytes(const")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    n, nodes, edges = C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    table = np.full(25, 7, dtype=U64)
    # a null handle
    assert lib.msbwt_rle_enumerate_kmer_graph(None, 3, 1, 0, None, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmer_graph_device(None, 3, 1, 0, None, None, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_kmer_graph_degrees(None, 3, 1, 0, _ptr(table), C.byref(nodes), C.byref(edges)) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, as everywhere in the API, so a bad k and a min_edge below the node threshold are
    # MSBWT_ERR_NOT_LOADED here; on a loaded index they are MSBWT_ERR_INVALID_ARG (tests/test_gpu_kmer_graph.py)
    b = msbwt.RleBWT()
    for k in (0, 3, 33):
        for min_count, min_edge in ((1, 0), (3, 2), (2, 5)):
            assert lib.msbwt_rle_enumerate_kmer_graph(b._h, k, min_count, min_edge, None, None, None, None, 0, C.byref(n)) == _lib.ERR_NOT_LOADED
            assert lib.msbwt_rle_enumerate_kmer_graph_device(b._h, k, min_count, min_edge, None, None, None, None, 0, C.byref(n), None) == _lib.ERR_NOT_LOADED
            assert lib.msbwt_rle_kmer_graph_degrees(b._h, k, min_count, min_edge, _ptr(table), C.byref(nodes), C.byref(edges)) == _lib.ERR_NOT_LOADED
            assert lib.msbwt_rle_kmer_graph_degrees(b._h, k, min_count, min_edge, None, None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (n.value, nodes.value, edges.value) == (77, 78, 79) and (table == 7).all()  # refused before anything was written
    with pytest.raises(msbwt.MsbwtError) as err:
        b.enumerate_kmer_graph(21)
    assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.kmer_graph_degrees(21, min_count=2, min_edge=3)
    assert err.value.code == _lib.ERR_NOT_LOADED
    assert b.spectrum_info()["k"] == 0 and b.spectrum_scratch_bytes() == 0


def test_plan_is_the_sorted_walks_plus_the_stated_terms():
    plan, walk = msbwt.kmer_graph_plan, msbwt.spectrum_plan
    rows = (0, 1, 1023, 1024, 1025, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 40 - 1)
    records = (0, 1, 2, 3, 4, 5, 7, 8, 10, 10 ** 6, 10 ** 6 + 1, 10 ** 9, 2 ** 40 - 1)
    for free in (0, 10 ** 9, FREE):
        for t in rows:
            for r in records:
                # the header's formula: the sorted walk, 256 bytes of degree counters, the edge bytes as whole 32-bit words, 24 per record
                assert plan(t, free, r) == walk(t, free, 0, True) + 256 + 4 * ((r + 3) // 4) + 24 * r, (t, free, r)
        sizes = [plan(t, free, 0) for t in rows]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], free
        for t in (10 ** 6, C4):
            sizes = [plan(t, free, r) for r in records]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(set(records)), (free, t)
    assert plan(C4, FREE) == plan(C4, FREE, 0)
    # the edge bytes are the cheap part: a byte per node against the 24 of its record
    assert plan(C4, FREE, 284 * 10 ** 6) - plan(C4, FREE, 0) == 25 * 284 * 10 ** 6


def test_plan_refuses_what_no_index_can_be():
    for t, r in ((2 ** 40, 0), (2 ** 40 + 1, 5), (2 ** 64 - 1, 0), (1000, 2 ** 40), (C4, 2 ** 64 - 1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.kmer_graph_plan(t, FREE, r)
        assert err.value.code == _lib.ERR_TOO_LARGE, (t, r)
    assert _lib.lib().msbwt_kmer_graph_plan(1000, FREE, 10, None) == 0  # the output is optional
    assert _lib.lib().msbwt_kmer_graph_plan(2 ** 40, FREE, 10, None) == _lib.ERR_TOO_LARGE


def word_of(kmer):
    w = 0
    for c in kmer:
        w = w << 2 | "ACGT".index(c)
    return w


def test_neighbour_helpers_on_hand_made_words_and_bytes():
    succ, pred = msbwt.rle_bwt.graph_successors, msbwt.rle_bwt.graph_predecessors
    k = 3
    words = np.array([word_of(q) for q in ("AAA", "ACG", "TTT", "GAT")], dtype=U64)
    #                 AAA: self-loop     ACG: <- G, T; -> T   TTT: nothing   GAT: <- A C G T; -> A C G T
    edges = np.array([0x01 | 0x10, 0x04 | 0x08 | 0x80, 0x00, 0xFF], dtype=np.uint8)
    at, nb = succ(words, edges, k)
    assert nb.dtype == U64 and at.tolist() == [0, 1, 3, 3, 3, 3]
    assert nb.tolist() == [word_of(q) for q in ("AAA", "CGT", "ATA", "ATC", "ATG", "ATT")]
    at, nb = pred(words, edges, k)
    assert nb.dtype == U64 and at.tolist() == [0, 1, 1, 3, 3, 3, 3]
    assert nb.tolist() == [word_of(q) for q in ("AAA", "GAC", "TAC", "AGA", "CGA", "GGA", "TGA")]
    # k = 1: the neighbour is the symbol itself; k = 32: the whole word moves, nothing above bit 63 survives
    at, nb = succ(np.array([2], dtype=U64), np.array([0x90], dtype=np.uint8), 1)
    assert at.tolist() == [0, 0] and nb.tolist() == [0, 3]
    at, nb = pred(np.array([2], dtype=U64), np.array([0x06], dtype=np.uint8), 1)
    assert at.tolist() == [0, 0] and nb.tolist() == [1, 2]
    q = "ACGT" * 8
    w32, e32 = np.array([word_of(q)], dtype=U64), np.array([0x22], dtype=np.uint8)
    assert succ(w32, e32, 32)[1].tolist() == [word_of(q[1:] + "C")] and pred(w32, e32, 32)[1].tolist() == [word_of("C" + q[:-1])]
    t31 = np.array([word_of("T" * 31)], dtype=U64)
    assert succ(t31, np.array([0x80], dtype=np.uint8), 31)[1].tolist() == [word_of("T" * 31)]
    # nothing set, nothing given
    for f in (succ, pred):
        at, nb = f(np.zeros(0, dtype=U64), np.zeros(0, dtype=np.uint8), 5)
        assert at.size == nb.size == 0
        at, nb = f(words, np.zeros(4, dtype=np.uint8), k)
        assert at.size == nb.size == 0
        for bad in (0, 33):
            with pytest.raises(ValueError):
                f(words, edges, bad)
        with pytest.raises(ValueError):
            f(words, edges[:3], k)


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "kmer_graph")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "kmer_graph.c"), "-o", exe] + _link_flags())
    for args in ([], ["-h"], ["x.npy", "0"], ["x.npy", "33"], ["x.npy", "21", "0"], ["x.npy", "21", "2", "more"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    if (msbwt::RleBWT::kmer_graph_plan(1000000, 0, 10) != msbwt::RleBWT::spectrum_plan(1000000, 0, 0, true) + 256 + 12 + 240) return 1;\n"
                   "    try { msbwt::RleBWT::kmer_graph_plan(std::uint64_t(1) << 40, 0); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    msbwt::RleBWT::KmerGraph (msbwt::RleBWT::*dump)(std::size_t, std::uint64_t, std::uint64_t) const = &msbwt::RleBWT::enumerate_kmer_graph;\n"
                   "    std::uint64_t (msbwt::RleBWT::*device)(std::size_t, std::uint64_t, std::uint64_t, void *, void *, void *, void *, std::uint64_t, void *) const =\n"
                   "        &msbwt::RleBWT::enumerate_kmer_graph_device;\n"
                   "    msbwt::RleBWT::GraphDegrees (msbwt::RleBWT::*degrees)(std::size_t, std::uint64_t, std::uint64_t) const = &msbwt::RleBWT::kmer_graph_degrees;\n"
                   "    msbwt::RleBWT::KmerGraph g;\n"
                   "    msbwt::RleBWT::GraphDegrees d;\n"
                   "    g.edges.push_back(std::uint8_t(0x11));\n"
                   "    return dump && device && degrees && g.words.empty() && sizeof d.table == 25 * 8 && d.nodes == 0 && d.edges == 0 ? 0 : 1;\n"
                   "}\n")
    exe = str(tmp_path / "mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe] + _link_flags())
    assert subprocess.run([exe]).returncode == 0


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in ("msbwt_rle_enumerate_kmer_graph", "msbwt_rle_kmer_graph_degrees", "msbwt_kmer_graph_plan"):
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn enumerate_kmer_graph(&self", "pub fn kmer_graph_degrees(&self", "pub fn kmer_graph_plan("):
            assert method in text
