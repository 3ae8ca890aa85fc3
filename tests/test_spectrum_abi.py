"""The spectrum and enumeration entry points (include/msbwt_hip.h: msbwt_rle_kmer_spectrum and its companions) without a GPU: the
symbols and their signatures, the guards that answer before a device is touched, the pure size plan, unpack_2bit, the example, the
C++ mirror and the shim's two copies."""
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
NEW = ("msbwt_rle_kmer_spectrum", "msbwt_rle_enumerate_kmers", "msbwt_rle_enumerate_kmers_device", "msbwt_rle_set_spectrum_frontier", "msbwt_rle_spectrum_info",
       "msbwt_spectrum_plan")
C4, HUMAN = 1_950_000_000, 90_000_000_000
FREE = 250 * 10 ** 9


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "void *": C.c_void_p, "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)),
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
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    assert "#define MSBWT_SPECTRUM_INFO_WORDS %d" % _lib.SPECTRUM_INFO_WORDS in header
    assert "#define MSBWT_SPECTRUM_MIN_FRONTIER %d" % _lib.SPECTRUM_MIN_FRONTIER in header
    assert header.index("msbwt_source_narrow_rows(") < header.index("msbwt_rle_kmer_spectrum(") < header.index("msbwt_rle_replicate(")  # a section of its own


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    hist, n = np.zeros(8, dtype=np.uint64), C.c_uint64(77)
    out = np.zeros(8, dtype=np.uint64)
    # a null handle
    assert lib.msbwt_rle_kmer_spectrum(None, 3, _ptr(hist), 8, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers(None, 3, 1, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_kmers_device(None, 3, 1, 0, 1, None, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_set_spectrum_frontier(None, 0) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_spectrum_info(None, _ptr(out)) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, as everywhere in the API (tests/test_capi_entry_guards.py), so k = 0 and 33, one bin
    # and min_count > max_count are refused with MSBWT_ERR_NOT_LOADED here; on a loaded index they are MSBWT_ERR_INVALID_ARG, which
    # needs a device to load one: tests/test_gpu_spectrum.py, test_argument_guards_on_a_loaded_index
    b = msbwt.RleBWT()
    for k in (0, 3, 33):
        assert lib.msbwt_rle_kmer_spectrum(b._h, k, _ptr(hist), 8, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_kmer_spectrum(b._h, k, _ptr(hist), 1, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_kmers(b._h, k, 1, 0, 1, None, None, None, 0, C.byref(n)) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_kmers_device(b._h, k, 5, 2, 1, None, None, None, 0, C.byref(n), None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    with pytest.raises(msbwt.MsbwtError) as err:
        b.kmer_spectrum(21)
    assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.enumerate_kmers(21)
    assert err.value.code == _lib.ERR_NOT_LOADED
    # the frontier knob needs no index
    for nodes in (1, _lib.SPECTRUM_MIN_FRONTIER - 1):
        assert lib.msbwt_rle_set_spectrum_frontier(b._h, nodes) == _lib.ERR_INVALID_ARG
        assert str(_lib.SPECTRUM_MIN_FRONTIER).encode() in lib.msbwt_rle_last_error(b._h)
    for nodes in (_lib.SPECTRUM_MIN_FRONTIER, 10 ** 6, 0):
        b.set_spectrum_frontier(nodes)
    assert _lib.SPECTRUM_MIN_FRONTIER >= 16  # a node's sixteen children fit
    info = b.spectrum_info()
    assert info["k"] == 0 and info["chunks"] == 0 and not info["nodes"].any() and len(info["nodes"]) == 33
    assert lib.msbwt_rle_spectrum_info(b._h, None) == _lib.ERR_INVALID_ARG


def test_plan_grows_with_rows_and_records_and_sorted_costs_more():
    plan = msbwt.spectrum_plan
    rows = (0, 1, 1023, 1024, 1025, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 40 - 1)
    for free in (0, 10 ** 9, FREE):
        for srt in (False, True):
            sizes = [plan(t, free, 0, srt) for t in rows]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (free, srt)
            for t in (10 ** 6, C4):
                sizes = [plan(t, free, r, srt) for r in (0, 1, 10, 10 ** 6, 10 ** 9)]
                assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (free, srt, t)
                assert plan(t, free, 10 ** 6, srt) - plan(t, free, 0, srt) == 24 * 10 ** 6  # k-mer, count, l
        for t in rows:
            assert plan(t, free, 0, True) >= plan(t, free, 0, False) + t // 8  # a bit per row at least
    # two frontiers of 24-byte nodes: never more than the rows can fill, 2^27 nodes at most
    assert plan(1000, FREE) < 2 * 24 * 5000 + 2 ** 16
    assert 2 * 24 * 2 ** 27 <= plan(HUMAN, 10 ** 12) < 2 * 24 * 2 ** 27 + 2 ** 16
    assert plan(C4, FREE, 0, True) < plan(C4, FREE) + C4 // 7  # the bitmap and its checkpoints: well under a byte per row


def test_plan_refuses_what_no_index_can_be():
    for t in (2 ** 40, 2 ** 40 + 1, 2 ** 64 - 1):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.spectrum_plan(t, FREE)
        assert err.value.code == _lib.ERR_TOO_LARGE
    assert _lib.lib().msbwt_spectrum_plan(1000, FREE, 0, 1, None) == 0  # the output is optional


@pytest.mark.parametrize("k", [1, 31, 32])
def test_unpack_2bit_inverts_pack_2bit(k):
    rng = np.random.default_rng(k)
    x = np.array([1, 2, 3, 5], dtype=np.uint8)[rng.integers(0, 4, size=(500, k))]
    x[0], x[1] = 1, 5  # A^k = 0 and T^k = all ones
    words = msbwt.rle_bwt.pack_2bit(x)
    assert words.shape == (500, 1) and words[0, 0] == 0 and words[1, 0] == (1 << 2 * k) - 1
    back = msbwt.rle_bwt.unpack_2bit(words, k)
    assert back.dtype == np.uint8 and np.array_equal(back, x)
    assert np.array_equal(msbwt.rle_bwt.unpack_2bit(words[:, 0], k), x) and msbwt.rle_bwt.unpack_2bit(np.zeros(0, dtype=np.uint64), k).shape == (0, k)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            msbwt.rle_bwt.unpack_2bit(words, bad)


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "kmer_spectrum")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "kmer_spectrum.c"), "-o", exe] + _link_flags())
    for args in ([], ["-h"], ["x.npy", "0"], ["x.npy", "33"], ["x.npy", "21", "more"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    if (msbwt::RleBWT::spectrum_plan(1000000, 0, 10, true) <= msbwt::RleBWT::spectrum_plan(1000000, 0)) return 1;\n"
                   "    try { msbwt::RleBWT::spectrum_plan(std::uint64_t(1) << 40, 0); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    msbwt::RleBWT::Spectrum (msbwt::RleBWT::*spectrum)(std::size_t, std::size_t) const = &msbwt::RleBWT::kmer_spectrum;\n"
                   "    msbwt::RleBWT::Kmers (msbwt::RleBWT::*dump)(std::size_t, std::uint64_t, std::uint64_t, bool) const = &msbwt::RleBWT::enumerate_kmers;\n"
                   "    std::uint64_t (msbwt::RleBWT::*device)(std::size_t, std::uint64_t, std::uint64_t, bool, void *, void *, void *, std::uint64_t, void *) const =\n"
                   "        &msbwt::RleBWT::enumerate_kmers_device;\n"
                   "    void (msbwt::RleBWT::*cap)(std::uint64_t) = &msbwt::RleBWT::set_spectrum_frontier;\n"
                   "    std::vector<std::uint64_t> (msbwt::RleBWT::*info)() const = &msbwt::RleBWT::spectrum_info;\n"
                   "    return spectrum && dump && device && cap && info ? 0 : 1;\n"
                   "}\n")
    exe = str(tmp_path / "mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe] + _link_flags())
    assert subprocess.run([exe]).returncode == 0


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in ("msbwt_rle_kmer_spectrum", "msbwt_rle_enumerate_kmers", "msbwt_rle_set_spectrum_frontier", "msbwt_spectrum_plan"):
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn kmer_spectrum(&self", "pub fn enumerate_kmers(&self", "pub fn set_spectrum_frontier(&mut self", "pub fn spectrum_plan("):
            assert method in text
