"""The unitig graph by source entry points (include/msbwt_hip.h: msbwt_rle_enumerate_[canonical_]unitig_graph_by_source[_device] and
their two plans) without a GPU: the symbols and their signatures, the guards that answer before a device is touched, the plans against
the terms the header states, the example, the C++ mirror, the shim's two copies and the sc:Z: tag of write_gfa."""
import ctypes as C
import importlib
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_unitigs_abi import C4, FREE, HUMAN, _link_flags

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
CALLS = ("msbwt_rle_enumerate_unitig_graph_by_source", "msbwt_rle_enumerate_unitig_graph_by_source_device",
         "msbwt_rle_enumerate_canonical_unitig_graph_by_source", "msbwt_rle_enumerate_canonical_unitig_graph_by_source_device")
NEW = CALLS + ("msbwt_unitig_graph_by_source_plan", "msbwt_canonical_unitig_graph_by_source_plan")
U64 = np.uint64
CHUNK = 1 << 20  # kCanonicalUnitigChunkSlots


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
        # the graph call's arguments in their order, one pointer more behind the link targets (the plans: n_sources before the output)
        old = _lib.SIGNATURES[name.replace("_by_source", "")][1]
        at = 7 if name.endswith("_plan") else 11
        assert args[:at - 1] + args[at:] == old and args[at - 1] == (C.c_size_t if name.endswith("_plan") else C.c_void_p), name
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own, behind the unitig links and before the scratch report; the definitions are in it
    assert header.index("msbwt_canonical_unitig_graph_plan(uint64_t") < header.index("---- unitigs by source ----") < header.index("msbwt_rle_enumerate_unitig_graph_by_source(")
    assert header.index("msbwt_canonical_unitig_graph_by_source_plan(uint64_t") < header.index("msbwt_rle_spectrum_scratch_bytes(const")
    section = header[header.index("---- unitigs by source ----"):header.index("msbwt_rle_enumerate_unitig_graph_by_source(")]
    for word in ("c_s(q)", "msbwt_rle_range_sources", "PLAIN CALL", "CANONICAL CALL", "c_s(q) + c_s(rc(q))", "ONCE", "ROW SUMS", "out_count_sums[u]", "THRESHOLDS",
                 "byte for byte", "writes NOTHING", "no sources attached", "U x S"):
        assert word in section, word
    assert "#define MSBWT_UNITIG_INFO_WORDS 8" in header and "#define MSBWT_CANONICAL_UNITIG_INFO_WORDS 10" in header


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    u, s, n = C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    bufs = [np.full(4, 7, dtype=t) for t in (np.uint8, U64, U64, np.uint8, np.uint8, U64, U64, U64)]
    ptrs, none = [_ptr(a) for a in bufs], (None,) * 8
    totals = (C.byref(u), C.byref(s), C.byref(n))
    b = msbwt.RleBWT()
    for name in CALLS:
        fn, stream = getattr(lib, name), ((None,) if name.endswith("_device") else ())
        # a null handle
        assert fn(None, 3, 1, 0, *ptrs, 4, 4, 4, *totals, *stream) == _lib.ERR_INVALID_ARG
        assert fn(None, 3, 1, 0, *none, 0, 0, 0, *totals, *stream) == _lib.ERR_INVALID_ARG
        # nothing loaded: the index is checked first, so a bad k, a min_edge below the node threshold and a missing *out_unitigs are
        # MSBWT_ERR_NOT_LOADED here; on a loaded index the attachment comes next (tests/test_gpu_unitig_sources.py)
        for k in (0, 3, 32, 33):
            for min_count, min_edge in ((1, 0), (3, 2), (2, 5)):
                assert fn(b._h, k, min_count, min_edge, *ptrs, 4, 4, 4, *totals, *stream) == _lib.ERR_NOT_LOADED
                assert fn(b._h, k, min_count, min_edge, *none, 0, 0, 0, None, None, None, *stream) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (u.value, s.value, n.value) == (77, 78, 79) and all((a == 7).all() for a in bufs)  # refused before anything was written
    for canonical in (False, True):
        with pytest.raises(msbwt.MsbwtError) as err:
            b.enumerate_unitig_graph_by_source(21, canonical=canonical)
        assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    for device in (b.enumerate_unitig_graph_by_source_device, b.enumerate_canonical_unitig_graph_by_source_device):
        with pytest.raises(msbwt.MsbwtError) as err:
            device(21, None, None, None, None, None, None, None, None, 0, 0, 0, min_count=2, min_edge=3)
        assert err.value.code == _lib.ERR_NOT_LOADED and (err.value.n, err.value.symbols, err.value.links) == (0, 0, 0)
    assert not any(b.unitig_info().values()) and not any(b.canonical_unitig_info().values())
    assert b.spectrum_info()["k"] == 0 and b.spectrum_scratch_bytes() == 0


def source_terms(n, u, sources, canonical):
    """the header's terms, one by one"""
    range_words = 2 * min(2 * n, CHUNK) if canonical else n
    return (8 * range_words + 255) // 256 * 256 + (8 * u * sources + 255) // 256 * 256


def test_plans_are_the_graph_plans_plus_the_stated_terms():
    rows = (0, 1, 1025, 10 ** 6, C4, HUMAN, 2 ** 40 - 1)
    records = (0, 1, 2, 5, 1023, 1024, 1025, 2047, 2048, 10 ** 6 + 1, 10 ** 9, 2 ** 40 - 1)
    for canonical in (False, True):
        old = lambda *a: msbwt.unitig_graph_plan(*a, canonical=canonical)
        for free in (0, FREE):
            for t in rows:
                for n in records:
                    for sources in (1, 4, 5, 32):
                        plan = lambda *a: msbwt.unitig_graph_by_source_plan(*a, n_sources=sources, canonical=canonical)
                        assert plan(t, free, n) == plan(t, free, n, 0, 0, 0) == old(t, free, n), (t, free, n)  # the counting call
                        for k in (1, 31):
                            for u in sorted({1, n // 30 + 1, max(n, 1)}):
                                s = n + u * (k - 1)
                                for links in (0, 2 * u + 1, 8 * u):
                                    assert plan(t, free, n, u, s, links) == old(t, free, n, u, s, links) + source_terms(n, u, sources, canonical), (t, free, n, u, s, links, sources)
    # C4 at k = 31 in 4 parts: 2.84e8 range words and 1e7 rows of 4
    assert msbwt.unitig_graph_by_source_plan(C4, FREE, 284 * 10 ** 6, 10 ** 7, 584 * 10 ** 6, 5 * 10 ** 7, n_sources=4) - \
        msbwt.unitig_graph_plan(C4, FREE, 284 * 10 ** 6, 10 ** 7, 584 * 10 ** 6, 5 * 10 ** 7) == 8 * 284 * 10 ** 6 + 32 * 10 ** 7
    assert msbwt.unitig_graph_by_source_plan(C4, FREE, 284 * 10 ** 6, 10 ** 7, 584 * 10 ** 6, 5 * 10 ** 7, n_sources=32, canonical=True) - \
        msbwt.unitig_graph_plan(C4, FREE, 284 * 10 ** 6, 10 ** 7, 584 * 10 ** 6, 5 * 10 ** 7, canonical=True) == 16 * CHUNK + 256 * 10 ** 7


def test_plans_refuse_what_no_index_can_be():
    for canonical in (False, True):
        for t, n, u, links in ((2 ** 40, 0, 0, 0), (2 ** 64 - 1, 0, 0, 0), (1000, 2 ** 40, 1, 1), (C4, 1000, 2 ** 40, 1), (C4, 1000, 10, 2 ** 43), (C4, 1000, 10, 2 ** 64 - 1)):
            with pytest.raises(msbwt.MsbwtError) as err:
                msbwt.unitig_graph_by_source_plan(t, FREE, n, u, n, links, n_sources=3, canonical=canonical)
            assert err.value.code == _lib.ERR_TOO_LARGE, (t, n, u, links)
        for sources in (0, 33, 2 ** 32):
            with pytest.raises(msbwt.MsbwtError) as err:
                msbwt.unitig_graph_by_source_plan(C4, FREE, 1000, 10, 1200, 4, n_sources=sources, canonical=canonical)
            assert err.value.code == _lib.ERR_INVALID_ARG, sources
    assert _lib.lib().msbwt_unitig_graph_by_source_plan(1000, FREE, 10, 2, 18, 4, 3, None) == 0  # the output is optional
    assert _lib.lib().msbwt_canonical_unitig_graph_by_source_plan(2 ** 40, FREE, 10, 2, 18, 4, 3, None) == _lib.ERR_TOO_LARGE
    assert _lib.lib().msbwt_canonical_unitig_graph_by_source_plan(1000, FREE, 10, 2, 18, 4, 0, None) == _lib.ERR_INVALID_ARG


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "unitigs_by_source")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "unitigs_by_source.c"), "-o", exe] + _link_flags())
    many = ["r%d.txt" % i for i in range(33)]
    for args in ([], ["-h"], ["--canonical"], ["21"], ["21", "2"], ["21", "2", "a.txt"], ["--canonical", "21", "2", "a.txt"], ["0", "2", "a.txt", "b.txt"],
                 ["33", "2", "a.txt", "b.txt"], ["--canonical", "32", "2", "a.txt", "b.txt"], ["21", "0", "a.txt", "b.txt"], ["a.txt", "b.txt", "21", "2"],
                 ["21", "2"] + many):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--canonical" in r.stderr and r.stdout == "", args
    readable = tmp_path / "reads.txt"
    readable.write_text("ACGT\n")
    r = subprocess.run([exe, "21", "2", str(readable), str(tmp_path / "no such file")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    using B = msbwt::RleBWT;\n"
                   "    if (B::unitig_graph_by_source_plan(1000000, 0, 10, 0, 0, 0, 4) != B::unitig_graph_plan(1000000, 0, 10)) return 1;\n"
                   "    if (B::unitig_graph_by_source_plan(1000000, 0, 10, 2, 18, 5, 4) != B::unitig_graph_plan(1000000, 0, 10, 2, 18, 5) + 256 + 256) return 1;\n"
                   "    if (B::unitig_graph_by_source_plan(1000000, 0, 10, 2, 18, 5, 32, true) != B::unitig_graph_plan(1000000, 0, 10, 2, 18, 5, true) + 512 + 512) return 1;\n"
                   "    try { B::unitig_graph_by_source_plan(1000, 0, 10, 2, 18, 5, 33); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_INVALID_ARG) return 1; }\n"
                   "    B::UnitigGraphBySource (B::*dump)(std::size_t, std::uint64_t, std::uint64_t, bool) const = &B::enumerate_unitig_graph_by_source;\n"
                   "    std::uint64_t (B::*device)(std::size_t, std::uint64_t, std::uint64_t, bool, void *, void *, void *, void *, void *, void *, void *, void *, std::uint64_t,\n"
                   "                               std::uint64_t, std::uint64_t, std::uint64_t *, std::uint64_t *, void *) const = &B::enumerate_unitig_graph_by_source_device;\n"
                   "    B::UnitigGraphBySource g;\n"
                   "    g.count_sums.push_back(4);\n"
                   "    g.link_offsets = {0, 1, 2};\n"
                   "    g.link_targets = {0, 1};\n"
                   "    g.sources = 2;\n"
                   "    g.source_sums = {1, 3};\n"
                   "    const B::UnitigGraph &base = g;\n"
                   "    return dump && device && base.size() == 1 && g.source_sums.size() == base.size() * g.sources ? 0 : 1;\n"
                   "}\n")
    exe = str(tmp_path / "mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe] + _link_flags())
    assert subprocess.run([exe]).returncode == 0


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in NEW:
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn enumerate_unitig_graph_by_source(&self", "pub unsafe fn enumerate_unitig_graph_by_source_device(&self", "pub fn unitig_graph_by_source_plan("):
            assert method in text


# what write_gfa wrote for this table before it knew of source_sums
TABLE = dict(k=3, symbols=np.array([1, 2, 3, 5, 2, 3, 5, 5], dtype=np.uint8), offsets=np.array([0, 4, 8], dtype=U64), count_sums=np.array([5, 2 ** 40], dtype=U64),
             flags=np.array([0, 2], dtype=np.uint8), link_offsets=np.array([0, 1, 2, 2, 2], dtype=U64), link_targets=np.array([2, 3], dtype=U64))
STORED = "H\tVN:Z:1.0\nS\t0\tACGT\tKC:i:5\nS\t1\tCGTT\tKC:i:1099511627776\nL\t0\t+\t1\t+\t2M\nL\t0\t-\t1\t-\t2M\n"


def test_write_gfa_without_the_matrix_is_what_it_was_and_with_it_carries_the_tag(tmp_path):
    from importlib import import_module
    rle_bwt = import_module("rust-msbwt_amd.rle_bwt")
    out = io.StringIO()
    assert rle_bwt.write_gfa(out, **TABLE) == (2, 2) and out.getvalue() == STORED
    out = io.StringIO()
    assert rle_bwt.write_gfa(out, **TABLE, source_sums=None) == (2, 2) and out.getvalue() == STORED
    path = str(tmp_path / "graph.gfa")
    matrix = np.array([[5, 0, 0], [1, 2 ** 40 - 3, 2]], dtype=U64)
    assert rle_bwt.write_gfa(path, **TABLE, source_sums=matrix) == (2, 2)
    lines = open(path).read().splitlines()
    assert lines[1] == "S\t0\tACGT\tKC:i:5\tsc:Z:5,0,0" and lines[2] == "S\t1\tCGTT\tKC:i:1099511627776\tsc:Z:1,1099511627773,2"
    assert [x for x in lines if not x.startswith("S")] == [x for x in STORED.splitlines() if not x.startswith("S")]
