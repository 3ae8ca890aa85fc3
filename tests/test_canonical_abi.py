"""The canonical k-mer entry points (include/msbwt_hip.h: msbwt_rle_canonical_kmer_spectrum and its companions) without a GPU: the
symbols and their signatures, the guards that answer before a device is touched, the pure reverse complement of packed words, the
pure size plan, the example, the C++ mirror and the shim's two copies."""
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
NEW = ("msbwt_kmers_reverse_complement_2bit", "msbwt_rle_canonical_kmer_spectrum", "msbwt_rle_enumerate_canonical_kmers",
       "msbwt_rle_enumerate_canonical_kmers_device", "msbwt_canonical_plan")
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
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    assert header.index("msbwt_spectrum_plan(") < header.index("msbwt_rle_canonical_kmer_spectrum(") < header.index("msbwt_rle_replicate(")  # a section of its own
    assert "sorted" not in ", ".join(decls["msbwt_rle_enumerate_canonical_kmers"][1]) and len(decls["msbwt_rle_enumerate_canonical_kmers"][1]) == 9


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    hist, n = np.zeros(8, dtype=U64), C.c_uint64(77)
    # a null handle
    assert lib.msbwt_rle_canonical_kmer_spectrum(None, 3, _ptr(hist), 8, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_canonical_kmers(None, 3, 1, 0, None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_canonical_kmers_device(None, 3, 1, 0, None, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, as everywhere in the API, so k = 0 and 33, one bin and min_count > max_count are refused
    # with MSBWT_ERR_NOT_LOADED here; on a loaded index they are MSBWT_ERR_INVALID_ARG, which needs a device to load one:
    # tests/test_gpu_canonical.py, test_capacity_pattern_of_both_forms
    b = msbwt.RleBWT()
    for k in (0, 3, 33):
        assert lib.msbwt_rle_canonical_kmer_spectrum(b._h, k, _ptr(hist), 8, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_canonical_kmer_spectrum(b._h, k, _ptr(hist), 1, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, k, 1, 0, None, None, None, 0, C.byref(n)) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_canonical_kmers(b._h, k, 5, 2, None, None, None, 0, C.byref(n)) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_enumerate_canonical_kmers_device(b._h, k, 5, 2, None, None, None, 0, C.byref(n), None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded" and n.value == 77 and not hist.any()
    for call in (lambda: b.canonical_kmer_spectrum(21), lambda: b.enumerate_canonical_kmers(21), lambda: b.enumerate_canonical_kmers(21, min_count=5, max_count=2),
                 lambda: b.enumerate_canonical_kmers_device(21, None, None, None, 0)):
        with pytest.raises(msbwt.MsbwtError) as err:
            call()
        assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    info = b.spectrum_info()
    assert info["k"] == 0 and info["chunks"] == 0 and not info["nodes"].any()


def _rc_by_symbols(words, k):
    """unpack, reverse_complement_i on the symbol codes, pack again"""
    syms = msbwt.rle_bwt.unpack_2bit(words, k)
    out = np.empty_like(syms)
    for i in range(len(syms)):
        _lib.lib().msbwt_reverse_complement_i(_ptr(np.ascontiguousarray(syms[i])), k, _ptr(out[i]))
    return msbwt.rle_bwt.pack_2bit(out)[:, 0]


@pytest.mark.parametrize("k", range(1, 33))
def test_reverse_complement_2bit_against_the_symbols(k):
    rng = np.random.default_rng(k)
    mask = U64((1 << 2 * k) - 1)
    words = rng.integers(0, 2 ** 64, size=300, dtype=U64) & mask
    words[0], words[1] = 0, mask  # A^k <-> T^k
    got = msbwt.rle_bwt.reverse_complement_2bit(words, k)
    assert got.dtype == U64 and got.shape == words.shape and got[0] == mask and got[1] == 0
    assert np.array_equal(got, _rc_by_symbols(words, k))
    assert np.array_equal(msbwt.rle_bwt.reverse_complement_2bit(got, k), words)  # an involution
    assert (got <= mask).all()
    dirty = words | ~mask  # bits above 2 k are ignored
    assert np.array_equal(msbwt.rle_bwt.reverse_complement_2bit(dirty, k), got)
    assert msbwt.rle_bwt.reverse_complement_2bit(words.reshape(-1, 1), k).shape == (300, 1)
    assert msbwt.rle_bwt.reverse_complement_2bit(np.zeros(0, dtype=U64), k).size == 0
    if k % 2:
        assert (got != words).all()  # no palindrome of odd length: the middle symbol is not its own complement
    else:
        pal = np.concatenate([words[:50] >> U64(k), U64(0) * words[:50]])[:50]  # a k/2-mer h, then rc(h) behind it
        pal = (pal << U64(k)) | msbwt.rle_bwt.reverse_complement_2bit(pal, k // 2)
        assert np.array_equal(msbwt.rle_bwt.reverse_complement_2bit(pal, k), pal)


def test_reverse_complement_2bit_refuses_other_k():
    lib = _lib.lib()
    words, out = np.arange(4, dtype=U64), np.full(4, 9, dtype=U64)
    for k in (0, 33, 64, 10 ** 6):
        assert lib.msbwt_kmers_reverse_complement_2bit(_ptr(words), k, 4, _ptr(out)) == _lib.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            msbwt.rle_bwt.reverse_complement_2bit(words, k)
    assert (out == 9).all()
    assert lib.msbwt_kmers_reverse_complement_2bit(None, 5, 4, _ptr(out)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_kmers_reverse_complement_2bit(_ptr(words), 5, 4, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_kmers_reverse_complement_2bit(None, 5, 0, None) == 0
    assert lib.msbwt_kmers_reverse_complement_2bit(_ptr(words), 2, 4, _ptr(words)) == 0 and words.tolist() == [15, 11, 7, 3]  # in place: AA AC AG AT -> TT GT CT AT


def test_plan_grows_with_rows_and_records_and_exceeds_the_plain_walk_by_the_staging():
    plan, plain = msbwt.canonical_plan, msbwt.spectrum_plan
    rows = (0, 1, 1023, 1024, 1025, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 40 - 1)
    for free in (0, 10 ** 9, FREE):
        sizes = [plan(t, free) for t in rows]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], free
        for t in (10 ** 6, C4):
            sizes = [plan(t, free, r) for r in (0, 1, 10, 10 ** 6, 10 ** 9)]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (free, t)
            assert plan(t, free, 10 ** 6) - plan(t, free) == 24 * 10 ** 6  # word, own, other
        for t in rows:
            walk = plain(t, free, 0, False)
            nodes = (walk - 32768) // 48  # two frontiers of 24-byte nodes behind the cursors and the re-seeding stack
            assert walk == 32768 + 48 * nodes and nodes >= 4096
            assert plan(t, free) == walk + 16 * nodes  # the other strand of a frontier's k-mers: word and count
    assert plan(1000, FREE) < 2 * (24 + 8) * 5000 + 2 ** 16
    assert (2 * 24 + 16) * 2 ** 27 <= plan(HUMAN, 10 ** 12) < (2 * 24 + 16) * 2 ** 27 + 2 ** 16


def test_plan_refuses_what_no_index_can_be():
    for t in (2 ** 40, 2 ** 40 + 1, 2 ** 64 - 1):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.canonical_plan(t, FREE)
        assert err.value.code == _lib.ERR_TOO_LARGE
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.canonical_plan(1000, FREE, t)
        assert err.value.code == _lib.ERR_TOO_LARGE
    assert _lib.lib().msbwt_canonical_plan(1000, FREE, 0, None) == 0  # the output is optional


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "canonical_spectrum")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "canonical_spectrum.c"), "-o", exe] + _link_flags())
    for args in ([], ["-h"], ["x.npy", "0"], ["x.npy", "33"], ["x.npy", "21", "0"], ["x.npy", "21", "2", "more"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    if (msbwt::RleBWT::canonical_plan(1000000, 0, 10) != msbwt::RleBWT::canonical_plan(1000000, 0) + 240) return 1;\n"
                   "    if (msbwt::RleBWT::canonical_plan(1000000, 0) <= msbwt::RleBWT::spectrum_plan(1000000, 0)) return 1;\n"
                   "    try { msbwt::RleBWT::canonical_plan(std::uint64_t(1) << 40, 0); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    const std::vector<std::uint64_t> rc = msbwt::RleBWT::reverse_complement_2bit({0, 1, 2, 3}, 2);\n"
                   "    if (rc != std::vector<std::uint64_t>{15, 11, 7, 3}) return 1;\n"
                   "    try { msbwt::RleBWT::reverse_complement_2bit({0}, 33); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_INVALID_ARG) return 1; }\n"
                   "    msbwt::RleBWT::Spectrum (msbwt::RleBWT::*spectrum)(std::size_t, std::size_t) const = &msbwt::RleBWT::canonical_kmer_spectrum;\n"
                   "    msbwt::RleBWT::CanonicalKmers (msbwt::RleBWT::*dump)(std::size_t, std::uint64_t, std::uint64_t) const = &msbwt::RleBWT::enumerate_canonical_kmers;\n"
                   "    return spectrum && dump ? 0 : 1;\n"
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
    for name in ("msbwt_kmers_reverse_complement_2bit", "msbwt_rle_canonical_kmer_spectrum", "msbwt_rle_enumerate_canonical_kmers", "msbwt_canonical_plan"):
        assert name in a and name in header, name
        assert len(a[name][1]) == len(header[name][1]), name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn canonical_kmer_spectrum(&self", "pub fn enumerate_canonical_kmers(&self", "pub fn reverse_complement_2bit(", "pub fn canonical_plan("):
            assert method in text
