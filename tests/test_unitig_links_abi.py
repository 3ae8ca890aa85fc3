"""The unitig graph entry points (include/msbwt_hip.h: msbwt_rle_enumerate_[canonical_]unitig_graph[_device] and their two plans)
without a GPU: the symbols and their signatures, the guards that answer before a device is touched, the plans against the terms the
header states, the example, the C++ mirror and the shim's two copies."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_unitigs_abi import C4, FREE, HUMAN, _link_flags

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
CALLS = ("msbwt_rle_enumerate_unitig_graph", "msbwt_rle_enumerate_unitig_graph_device", "msbwt_rle_enumerate_canonical_unitig_graph",
         "msbwt_rle_enumerate_canonical_unitig_graph_device")
NEW = CALLS + ("msbwt_unitig_graph_plan", "msbwt_canonical_unitig_graph_plan")
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
    # a section of its own, behind the canonical unitigs and before the scratch report; the definitions are in it
    assert header.index("msbwt_canonical_unitigs_plan(uint64_t") < header.index("---- unitig links ----") < header.index("msbwt_rle_enumerate_unitig_graph(")
    assert header.index("msbwt_canonical_unitig_graph_plan(uint64_t") < header.index("msbwt_rle_spectrum_scratch_bytes(const")
    section = header[header.index("---- unitig links ----"):header.index("msbwt_rle_enumerate_unitig_graph(")]
    for word in ("SIDES", "ENTRIES", "PLAIN CALL", "CANONICAL CALL", "MIRROR RECORDS", "2v + o", "L = 2 (edges - links + circular)", "ONE side", "writes NOTHING"):
        assert word in section, word
    # the existing unitig declarations and their info words stand as they were
    assert "#define MSBWT_UNITIG_INFO_WORDS 8" in header and "#define MSBWT_CANONICAL_UNITIG_INFO_WORDS 10" in header


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    u, s, n = C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    bufs = [np.full(4, 7, dtype=t) for t in (np.uint8, U64, U64, np.uint8, np.uint8, U64, U64)]
    ptrs, none = [_ptr(a) for a in bufs], (None,) * 7
    totals = (C.byref(u), C.byref(s), C.byref(n))
    b = msbwt.RleBWT()
    for name in CALLS:
        fn, stream = getattr(lib, name), ((None,) if name.endswith("_device") else ())
        # a null handle
        assert fn(None, 3, 1, 0, *ptrs, 4, 4, 4, *totals, *stream) == _lib.ERR_INVALID_ARG
        assert fn(None, 3, 1, 0, *none, 0, 0, 0, *totals, *stream) == _lib.ERR_INVALID_ARG
        # nothing loaded: the index is checked first, as everywhere in the API, so a bad k, a min_edge below the node threshold and a
        # missing *out_unitigs are MSBWT_ERR_NOT_LOADED here; on a loaded index they are MSBWT_ERR_INVALID_ARG (tests/test_gpu_unitig_links.py)
        for k in (0, 3, 32, 33):
            for min_count, min_edge in ((1, 0), (3, 2), (2, 5)):
                assert fn(b._h, k, min_count, min_edge, *ptrs, 4, 4, 4, *totals, *stream) == _lib.ERR_NOT_LOADED
                assert fn(b._h, k, min_count, min_edge, *none, 0, 0, 0, None, None, None, *stream) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (u.value, s.value, n.value) == (77, 78, 79) and all((a == 7).all() for a in bufs)  # refused before anything was written
    for canonical in (False, True):
        with pytest.raises(msbwt.MsbwtError) as err:
            b.enumerate_unitig_graph(21, canonical=canonical)
        assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    for device in (b.enumerate_unitig_graph_device, b.enumerate_canonical_unitig_graph_device):
        with pytest.raises(msbwt.MsbwtError) as err:
            device(21, None, None, None, None, None, None, None, 0, 0, 0, min_count=2, min_edge=3)
        assert err.value.code == _lib.ERR_NOT_LOADED and (err.value.n, err.value.symbols, err.value.links) == (0, 0, 0)
    assert not any(b.unitig_info().values()) and not any(b.canonical_unitig_info().values())
    assert b.spectrum_info()["k"] == 0 and b.spectrum_scratch_bytes() == 0


def link_terms(u, links):
    """the header's terms, one by one"""
    return 16 * u + 256 + 16 * ((2 * u + 1 + 2047) // 2048) + 8 * links


def test_plans_are_the_unitig_plans_plus_the_stated_terms():
    rows = (0, 1, 1025, 10 ** 6, C4, HUMAN, 2 ** 40 - 1)
    records = (0, 1, 2, 5, 1023, 1024, 1025, 2047, 2048, 10 ** 6 + 1, 10 ** 9, 2 ** 40 - 1)
    for canonical, old in ((False, msbwt.unitigs_plan), (True, msbwt.canonical_unitigs_plan)):
        plan = lambda *a: msbwt.unitig_graph_plan(*a, canonical=canonical)
        for free in (0, FREE):
            for t in rows:
                for n in records:
                    assert plan(t, free, n) == plan(t, free, n, 0, 0, 0) == old(t, free, n), (t, free, n)  # the counting call
                    for k in (1, 21, 31):
                        for u in sorted({1, n // 30 + 1, max(n, 1)}):
                            s = n + u * (k - 1)
                            for links in (0, 1, u, 2 * u + 1, 8 * u):
                                assert plan(t, free, n, u, s, links) == old(t, free, n, u, s) + link_terms(u, links), (t, free, n, u, s, links)
    # C4 at k = 31: 5e7 entries on 1e7 unitigs
    assert msbwt.unitig_graph_plan(C4, FREE, 284 * 10 ** 6, 10 ** 7, 584 * 10 ** 6, 5 * 10 ** 7) - msbwt.unitigs_plan(C4, FREE, 284 * 10 ** 6, 10 ** 7, 584 * 10 ** 6) == \
        16 * 10 ** 7 + 256 + 16 * 9766 + 4 * 10 ** 8


def test_plans_refuse_what_no_index_can_be():
    for canonical in (False, True):
        for t, n, u, links in ((2 ** 40, 0, 0, 0), (2 ** 64 - 1, 0, 0, 0), (1000, 2 ** 40, 1, 1), (C4, 1000, 2 ** 40, 1), (C4, 1000, 10, 2 ** 43), (C4, 1000, 10, 2 ** 64 - 1)):
            with pytest.raises(msbwt.MsbwtError) as err:
                msbwt.unitig_graph_plan(t, FREE, n, u, n, links, canonical=canonical)
            assert err.value.code == _lib.ERR_TOO_LARGE, (t, n, u, links)
    assert _lib.lib().msbwt_unitig_graph_plan(1000, FREE, 10, 2, 18, 4, None) == 0  # the output is optional
    assert _lib.lib().msbwt_canonical_unitig_graph_plan(2 ** 40, FREE, 10, 2, 18, 4, None) == _lib.ERR_TOO_LARGE


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "unitigs_gfa")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "unitigs_gfa.c"), "-o", exe] + _link_flags())
    for args in ([], ["-h"], ["--canonical"], ["reads.txt"], ["reads.txt", "0"], ["reads.txt", "33"], ["--canonical", "reads.txt", "32"], ["reads.txt", "21", "0"],
                 ["reads.txt", "21", "2", "more"], ["--canonical", "reads.txt", "21", "2", "more"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--canonical" in r.stderr and r.stdout == "", args
    r = subprocess.run([exe, str(tmp_path / "no such file"), "21"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    using B = msbwt::RleBWT;\n"
                   "    if (B::unitig_graph_plan(1000000, 0, 10) != B::unitigs_plan(1000000, 0, 10)) return 1;\n"
                   "    if (B::unitig_graph_plan(1000000, 0, 10, 2, 18, 5) != B::unitigs_plan(1000000, 0, 10, 2, 18) + 32 + 256 + 16 + 40) return 1;\n"
                   "    if (B::unitig_graph_plan(1000000, 0, 10, 2, 18, 5, true) != B::canonical_unitigs_plan(1000000, 0, 10, 2, 18) + 32 + 256 + 16 + 40) return 1;\n"
                   "    try { B::unitig_graph_plan(1000, 0, 10, 2, 18, std::uint64_t(1) << 43); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    B::UnitigGraph (B::*dump)(std::size_t, std::uint64_t, std::uint64_t, bool) const = &B::enumerate_unitig_graph;\n"
                   "    std::uint64_t (B::*device)(std::size_t, std::uint64_t, std::uint64_t, bool, void *, void *, void *, void *, void *, void *, void *, std::uint64_t,\n"
                   "                               std::uint64_t, std::uint64_t, std::uint64_t *, std::uint64_t *, void *) const = &B::enumerate_unitig_graph_device;\n"
                   "    B::UnitigGraph g;\n"
                   "    g.count_sums.push_back(4);\n"
                   "    g.link_offsets = {0, 1, 2};\n"
                   "    g.link_targets = {0, 1};\n"
                   "    const B::Unitigs &base = g;\n"
                   "    return dump && device && base.size() == 1 && g.link_offsets.back() == g.link_targets.size() ? 0 : 1;\n"
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
        for method in ("pub fn enumerate_unitig_graph(&self", "pub unsafe fn enumerate_unitig_graph_device(&self", "pub fn unitig_graph_plan("):
            assert method in text
