"""The source-colouring entry points (include/msbwt_hip.h: msbwt_rle_set_sources and its companions) without a GPU: the symbols and
their signatures, the pure size plan and its documented bound, the guards that answer before a device is touched, the example, the
shim's two copies."""
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
NEW = ("msbwt_rle_set_sources", "msbwt_rle_load_merged_many_sources", "msbwt_rle_source_count", "msbwt_rle_source_totals",
       "msbwt_rle_count_kmers_by_source", "msbwt_rle_count_kmers_by_source_device", "msbwt_rle_range_sources", "msbwt_rle_range_sources_device",
       "msbwt_source_index_plan", "msbwt_source_block_rows", "msbwt_source_narrow_rows")
C4, HUMAN = 3_900_000_000, 90_000_000_000


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "const uint8_t *": C.c_void_p, "const uint64_t *": C.c_void_p,
                "const void *": C.c_void_p, "void *": C.c_void_p, "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "size_t": C.c_size_t,
                "uint64_t": C.c_uint64, "int": C.c_int}
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
    assert "#define MSBWT_SOURCE_INDEX_SLACK %d" % _lib.SOURCE_INDEX_SLACK in header
    assert header.index("msbwt_rle_merge_info(") < header.index("msbwt_rle_set_sources(") < header.index("msbwt_rle_replicate(")  # after the merge section


def test_block_rows_is_a_power_of_two_and_the_narrow_path_lies_inside_a_block():
    rows, narrow = msbwt.source_block_rows(), msbwt.source_narrow_rows()
    assert rows >= 64 and rows & (rows - 1) == 0
    assert 16 <= narrow < rows


def test_plan_is_monotone_in_both_arguments():
    plan = msbwt.source_index_plan
    rows = msbwt.source_block_rows()
    steps = (0, 1, rows - 1, rows, rows + 1, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 40 - 1)
    for n in range(1, 33):
        sizes = [plan(t, n) for t in steps]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], n
    for t in steps:
        sizes = [plan(t, n) for n in range(1, 33)]
        assert sizes == sorted(sizes), t
        assert sizes[0] >= t  # the byte per row is always there
    assert plan(HUMAN, 32) > plan(HUMAN, 16) > plan(HUMAN, 1)


def test_plan_stays_within_the_documented_bound():
    plan = msbwt.source_index_plan
    rows = msbwt.source_block_rows()
    for t in (0, 1, 255, 256, rows - 1, rows, rows + 1, 2 * rows + 1, 10 ** 6 + 7, C4, HUMAN, 2 ** 40 - 1):
        for n in (1, 2, 3, 8, 16, 17, 32):
            assert t <= plan(t, n) <= 1.5 * t + _lib.SOURCE_INDEX_SLACK, (t, n)
        assert plan(t, 32) * 2 <= 3 * t + 2 * _lib.SOURCE_INDEX_SLACK  # the same bound in integers: no rounding of a float at 2^40
    up = lambda x, m: (x + m - 1) // m * m
    for t in (0, 1, rows, rows + 1, 10 ** 6 + 7):  # the layout itself: the padded byte vector, and a checkpoint of 8-byte counters before every block and after the last
        for n in (1, 2, 3, 8, 17, 32):
            stride = 1 << (n - 1).bit_length()
            assert plan(t, n) == up(t, 256) + up((up(t, rows) // rows + 1) * stride * 8, 256), (t, n)
    assert plan(HUMAN, 4) < 1.04 * HUMAN and plan(HUMAN, 32) < 1.26 * HUMAN


def test_plan_refuses_what_no_attachment_can_be():
    plan = msbwt.source_index_plan
    for t in (2 ** 40, 2 ** 40 + 1, 2 ** 64 - 1):
        with pytest.raises(msbwt.MsbwtError) as err:
            plan(t, 3)
        assert err.value.code == _lib.ERR_TOO_LARGE
    for n in (0, 33, 1000):
        with pytest.raises(msbwt.MsbwtError) as err:
            plan(1000, n)
        assert err.value.code == _lib.ERR_INVALID_ARG
    assert _lib.lib().msbwt_source_index_plan(1000, 3, None) == 0  # the output is optional


def test_guards_answer_without_a_device():
    b = msbwt.RleBWT()
    assert b.source_count() == 0
    sources = np.zeros(4, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    lib = _lib.lib()
    assert lib.msbwt_rle_set_sources(b._h, sources.ctypes.data_as(C.c_void_p), 4, 1) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_source_totals(b._h, out.ctypes.data_as(C.c_void_p)) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_count_kmers_by_source(b._h, sources.ctypes.data_as(C.c_void_p), 2, 2, out.ctypes.data_as(C.c_void_p)) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_range_sources(b._h, out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_count_kmers_by_source_device(b._h, None, 2, 2, None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_range_sources_device(b._h, None, None, 1, None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_source_count(None) == 0
    for call in (lambda: lib.msbwt_rle_set_sources(None, None, 0, 0), lambda: lib.msbwt_rle_source_totals(None, None),
                 lambda: lib.msbwt_rle_count_kmers_by_source(None, None, 0, 0, None), lambda: lib.msbwt_rle_range_sources(None, None, None, 0, None),
                 lambda: lib.msbwt_rle_load_merged_many_sources(None, None, None, 0)):
        assert call() == _lib.ERR_INVALID_ARG
    ok = np.array([1 | 3 << 3, 0 | 1 << 3], dtype=np.uint8)
    for rles, code in (([ok] * 33, _lib.ERR_INVALID_ARG), ([ok, [6 | 1 << 3]], _lib.ERR_INVALID_SYMBOL), ([ok, [0xF9] * 9], _lib.ERR_TOO_LARGE)):
        with pytest.raises(msbwt.MsbwtError) as err:
            b.load_merged_many(rles, keep_sources=True)
        assert err.value.code == code
    with pytest.raises(ValueError):
        msbwt.bwt_util.merge_numpy_files([], "nowhere.npy", sources_out="nowhere.sources.npy")


def _compile(src, out, std):
    subprocess.check_call(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", LIBDIR,
                           "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "count_by_source")
    _compile(os.path.join(ROOT, "examples", "count_by_source.c"), exe, "c11")
    for args in ([], ["-h"], ["ACG", "T"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    if (msbwt::RleBWT::source_block_rows() != msbwt_source_block_rows()) return 1;\n"
                   "    if (msbwt::RleBWT::source_index_plan(1000, 3) < 1000) return 1;\n"
                   "    if (msbwt::RleBWT::source_narrow_rows() != msbwt_source_narrow_rows()) return 1;\n"
                   "    try { msbwt::RleBWT::source_index_plan(1000, 33); return 1; } catch (const msbwt::Panic &) {}\n"
                   "    void (msbwt::RleBWT::*attach)(const std::vector<std::uint8_t> &, std::size_t) = &msbwt::RleBWT::set_sources;\n"
                   "    std::vector<std::uint64_t> (msbwt::RleBWT::*count)(const std::vector<std::uint8_t> &, std::size_t) const = &msbwt::RleBWT::count_kmers_by_source;\n"
                   "    return attach && count ? 0 : 1;\n"
                   "}\n")
    exe = str(tmp_path / "mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", LIBDIR, "-lmsbwt_hip",
                           "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    assert subprocess.run([exe]).returncode == 0


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in ("msbwt_rle_set_sources", "msbwt_rle_load_merged_many_sources", "msbwt_rle_source_count", "msbwt_rle_source_totals",
                 "msbwt_rle_count_kmers_by_source", "msbwt_rle_range_sources", "msbwt_source_index_plan"):
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn set_sources(&mut self", "pub fn load_merged_many_sources(&mut self", "pub fn count_kmers_by_source(&self", "pub fn range_sources(&self"):
            assert method in text
