"""The k-mers-by-source entry points (include/msbwt_hip.h: msbwt_rle_kmer_spectrum_by_source and its companions) without a GPU: the
symbols and their signatures, the guards that answer before a device is touched, the pure size plan -- which must not hold a term of
frontier x sources --, the example, the C++ mirror and the shim's two copies."""
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
NEW = ("msbwt_rle_kmer_spectrum_by_source", "msbwt_rle_enumerate_kmers_by_source", "msbwt_rle_enumerate_kmers_by_source_device", "msbwt_kmers_by_source_plan",
       "msbwt_rle_spectrum_scratch_bytes")
C4, HUMAN = 1_950_000_000, 90_000_000_000
FREE = 250 * 10 ** 9
U64 = np.uint64


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"const msbwt_rle *": C.c_void_p, "void *": C.c_void_p, "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "const uint64_t *": C.c_void_p,
                "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int": C.c_int}
    for name in NEW:
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SIGNATURES[name]
        cret, cparams = decls[name]
        assert ctype_of[shim.norm_c(cret)] == res, name
        assert len(cparams) == len(args), name
        for ct, a in zip(cparams, args):
            want = ctype_of[shim.norm_c(ct)]
            assert a in want if isinstance(want, tuple) else a == want, (name, ct)
    assert len(decls["msbwt_rle_kmer_spectrum_by_source"][1]) == 7
    assert len(decls["msbwt_rle_enumerate_kmers_by_source"][1]) == 12 and len(decls["msbwt_rle_enumerate_kmers_by_source_device"][1]) == 13
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own, after the canonical one and before the multi-GPU one
    assert header.index("msbwt_canonical_plan(") < header.index("msbwt_rle_kmer_spectrum_by_source(") < header.index("msbwt_kmers_by_source_plan(") \
        < header.index("msbwt_rle_spectrum_scratch_bytes(") < header.index("msbwt_rle_replicate(")
    section = header[header.index("k-mers by source"):header.index("msbwt_rle_replicate(")]
    assert "0 means ABSENT FROM THIS SOURCE" in section and "deliberately differs" in section  # the convention of max_counts is spelt out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    hist, n = np.zeros(8, dtype=U64), C.c_uint64(77)
    words = np.full(4, 9, dtype=U64)
    lo, hi = np.array([5, 0], dtype=U64), np.array([2, 0], dtype=U64)  # min > max
    # a null handle
    assert lib.msbwt_rle_kmer_spectrum_by_source(None, 3, _ptr(hist), 8, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers_by_source(None, 3, None, None, 1, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers_by_source_device(None, 3, None, None, 1, 0, 1, None, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, as everywhere in the API, so k = 0 and 33, one bin, min > max and a total window the wrong
    # way round are refused with MSBWT_ERR_NOT_LOADED here; on a loaded index they are MSBWT_ERR_INVALID_ARG, which needs a device to load one:
    # tests/test_gpu_source_spectrum.py, test_predicates
    b = msbwt.RleBWT()
    for k in (0, 3, 33):
        assert lib.msbwt_rle_kmer_spectrum_by_source(b._h, k, _ptr(hist), 8, None, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_kmer_spectrum_by_source(b._h, k, _ptr(hist), 1, None, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, k, None, None, 1, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, k, _ptr(lo), _ptr(hi), 1, 0, 1, _ptr(words), None, None, 4, C.byref(n)) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_kmers_by_source(b._h, k, None, None, 5, 2, 0, _ptr(words), None, None, 4, C.byref(n)) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_kmers_by_source_device(b._h, k, _ptr(lo), _ptr(hi), 5, 2, 1, None, None, None, 0, C.byref(n), None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert n.value == 77 and not hist.any() and (words == 9).all()  # *out_n and the buffers untouched
    assert b.source_count() == 0
    for call in (lambda: b.kmer_spectrum_by_source(21), lambda: b.enumerate_kmers_by_source(21), lambda: b.enumerate_kmers_by_source(21, min_total=5, max_total=2),
                 lambda: b.enumerate_kmers_by_source_device(21, None, None, None, 0)):
        with pytest.raises(msbwt.MsbwtError) as err:
            call()
        assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    info = b.spectrum_info()
    assert info["k"] == 0 and info["chunks"] == 0 and not info["nodes"].any()
    assert b.spectrum_scratch_bytes() == 0  # no walk has run
    assert lib.msbwt_rle_spectrum_scratch_bytes(None, C.byref(n)) == _lib.ERR_INVALID_ARG and lib.msbwt_rle_spectrum_scratch_bytes(b._h, None) == _lib.ERR_INVALID_ARG
    assert n.value == 77


def test_plan_is_the_walk_plus_a_fixed_term_plus_the_staged_records():
    plan, plain = msbwt.kmers_by_source_plan, msbwt.spectrum_plan
    rows = (0, 1, 1023, 1024, 1025, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 40 - 1)
    fixed = set()
    for free in (0, 10 ** 9, FREE, 10 ** 12):
        for s in (1, 4, 32):
            for srt in (False, True):
                sizes = [plan(t, free, s, 0, srt) for t in rows]
                assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (free, s, srt)  # monotone in rows
                for t in rows:
                    # what the plain walk takes, and a term that is the same at every size, every frontier and every number of sources
                    fixed.add(plan(t, free, s, 0, srt) - plain(t, free, 0, srt))
            for t in (10 ** 6, C4):
                sizes = [plan(t, free, s, r) for r in (0, 1, 10, 10 ** 6, 10 ** 9)]
                assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (free, t, s)  # monotone in records
                assert plan(t, free, s, 10 ** 6) - plan(t, free, s) == 8 * (2 + s) * 10 ** 6  # word, l and S counts, for a host dump alone
    assert len(fixed) == 1 and 0 < fixed.pop() <= 4096
    # the automatic frontier at its largest: 2^27 nodes of 24 bytes, twice -- and nothing per node and source (34 GB at 32 sources)
    for s in (1, 32):
        assert 2 * 24 * 2 ** 27 <= plan(HUMAN, 10 ** 12, s) < 2 * 24 * 2 ** 27 + 2 ** 16
    assert plan(HUMAN, 10 ** 12, 32) == plan(HUMAN, 10 ** 12, 1)
    assert plan(1000, FREE, 32) < 2 * 24 * 5000 + 2 ** 16


def test_plan_refuses_what_no_index_can_be():
    for t in (2 ** 40, 2 ** 40 + 1, 2 ** 64 - 1):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.kmers_by_source_plan(t, FREE, 4)
        assert err.value.code == _lib.ERR_TOO_LARGE
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.kmers_by_source_plan(1000, FREE, 4, t)
        assert err.value.code == _lib.ERR_TOO_LARGE
    for s in (0, 33, 10 ** 6):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.kmers_by_source_plan(1000, FREE, s)
        assert err.value.code == _lib.ERR_INVALID_ARG
    assert _lib.lib().msbwt_kmers_by_source_plan(1000, FREE, 4, 0, 1, None) == 0  # the output is optional


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "private_kmers")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "private_kmers.c"), "-o", exe] + _link_flags())
    for args in (["-h"], ["0"], ["33"], ["3", "more"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    using B = msbwt::RleBWT;\n"
                   "    if (B::kmers_by_source_plan(1000000, 0, 4, 10) != B::kmers_by_source_plan(1000000, 0, 4) + 480) return 1;\n"
                   "    if (B::kmers_by_source_plan(1000000, 0, 32) != B::kmers_by_source_plan(1000000, 0, 1)) return 1;\n"
                   "    if (B::kmers_by_source_plan(1000000, 0, 4, 0, true) <= B::spectrum_plan(1000000, 0, 0, true)) return 1;\n"
                   "    try { B::kmers_by_source_plan(std::uint64_t(1) << 40, 0, 4); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    try { B::kmers_by_source_plan(1000, 0, 33); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_INVALID_ARG) return 1; }\n"
                   "    if (B::kNoLimit != UINT64_MAX) return 1;\n"
                   "    B::SourceSpectrum (B::*spectrum)(std::size_t, std::size_t) const = &B::kmer_spectrum_by_source;\n"
                   "    B::SourceKmers (B::*dump)(std::size_t, const std::vector<std::uint64_t> &, const std::vector<std::uint64_t> &, std::uint64_t, std::uint64_t, bool) const =\n"
                   "        &B::enumerate_kmers_by_source;\n"
                   "    auto device = &B::enumerate_kmers_by_source_device;\n"
                   "    std::uint64_t (B::*scratch)() const = &B::spectrum_scratch_bytes;\n"
                   "    return spectrum && dump && device && scratch ? 0 : 1;\n"
                   "}\n")
    exe = str(tmp_path / "mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe] + _link_flags())
    assert subprocess.run([exe]).returncode == 0


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    header = shim.c_declarations()
    for name in ("msbwt_rle_kmer_spectrum_by_source", "msbwt_rle_enumerate_kmers_by_source", "msbwt_kmers_by_source_plan", "msbwt_rle_spectrum_scratch_bytes"):
        assert name in a and name in header, name
        assert len(a[name][1]) == len(header[name][1]), name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn kmer_spectrum_by_source(&self", "pub fn enumerate_kmers_by_source(&self", "pub fn kmers_by_source_plan(", "pub fn spectrum_scratch_bytes(&self"):
            assert method in text
