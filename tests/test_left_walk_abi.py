"""The left-walk entry points (include/msbwt_hip.h, "left walks": msbwt_rle_walk_rows[_device], msbwt_rle_extract_reads[_device],
msbwt_rle_walk_info, msbwt_rle_set_walk_piece, msbwt_walk_plan) without a GPU: the symbols and their signatures, the header section's
place, key words and stop codes, the guards that answer before a device is touched, the pure size plan against the terms the header
states, walk_sequences on hand-written arrays, the example, the C++ mirror and the shim's two copies."""
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
NEW = ("msbwt_rle_walk_rows", "msbwt_rle_walk_rows_device", "msbwt_rle_extract_reads", "msbwt_rle_extract_reads_device", "msbwt_rle_walk_info",
       "msbwt_rle_set_walk_piece", "msbwt_walk_plan")
U64 = np.uint64


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p,
                "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "const uint64_t *": C.c_void_p, "uint8_t *": C.c_void_p, "size_t": C.c_size_t,
                "uint64_t": C.c_uint64, "int": C.c_int}
    for name in NEW:
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SIGNATURES[name]
        cret, cparams = decls[name]
        assert ctype_of[shim.norm_c(cret)] == res, name
        assert len(cparams) == len(args), name
        for ct, a in zip(cparams, args):
            assert shim.norm_c(ct) in shim.C_TO_RUST, (name, ct)  # only the C types the shim test knows
            want = ctype_of[shim.norm_c(ct)]
            assert a in want if isinstance(want, tuple) else a == want, (name, ct)
    assert [len(decls[name][1]) for name in NEW] == [9, 10, 10, 11, 2, 2, 6]


def test_header_section():
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own behind the canonical traces, before "several GPUs"
    assert header.index("---- canonical traces ----") < header.index("msbwt_canonical_trace_plan(uint64_t") < header.index("---- left walks ----")
    assert header.index("---- left walks ----") < header.index("msbwt_rle_walk_rows(") < header.index("msbwt_walk_plan(uint64_t") < header.index("---- several GPUs")
    section = header[header.index("---- left walks ----"):header.index("---- several GPUs")]
    prose = " ".join(line.strip().lstrip("*").strip() for line in section.splitlines())  # the comment's lines joined: a phrase may wrap
    for word in ("LF(r) = C[S[r]] + rank(S[r], r)", "start_index", "BAD_ROW", "DOLLAR", "MAX_STEPS", "neither emitted nor counted", "LAST SYMBOL FIRST", "an empty read first",
                 "duplicates in input order", "rank('$', r_p)", "left untouched", "needs no alignment", "LOCATE", "UINT64_MAX", "MSBWT_ERR_INVALID_RANGE",
                 "msbwt_rle_constrain_ranges", "msbwt_rle_device_status", "MSBWT_ERR_TOO_LARGE", "2^40", "READING order", "msbwt_rle_count_ragged_read_kmers",
                 "msbwt_rle_build_from_reads", "LAST max_len symbols", "the message names S", "unspecified within its capacity", "nothing is written past it",
                 "THE WALK IS THE WHOLE COST", "n x max_len", "ONE 128-byte line", "2^20", "EXACTLY", "pad(P max_steps)", "sampled", "right walks", "per-source",
                 "several GPUs", "DESIGN.md", "any loaded stream", "msbwt_rle_device_bytes unchanged", "in this order", "no BWT loaded"):
        assert word in prose, word
    assert "uint32_t" not in section
    values = dict(line.split()[2:4] for line in section.splitlines() if line.startswith("#  define MSBWT_WALK_"))
    assert values == {"MSBWT_WALK_DOLLAR": "1", "MSBWT_WALK_MAX_STEPS": "2", "MSBWT_WALK_BAD_ROW": "3", "MSBWT_WALK_INFO_WORDS": "8"}
    assert _lib.WALK_INFO_WORDS == 8 and _lib.WALK_STOPS == ("", "DOLLAR", "MAX_STEPS", "BAD_ROW")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    rows, steps = np.array([5, 6], dtype=U64), np.full(3, 77, dtype=U64)
    info = np.full(8, 9, dtype=U64)
    total, truncated = C.c_uint64(99), C.c_uint64(99)
    # a null handle
    assert lib.msbwt_rle_walk_rows(None, _ptr(rows), 2, 4, None, _ptr(steps), None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_walk_rows_device(None, None, 0, 4, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_extract_reads(None, None, 0, 2, 4, None, _ptr(steps), 0, C.byref(total), C.byref(truncated)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_extract_reads_device(None, None, 0, 2, 4, None, None, 0, C.byref(total), None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_walk_info(None, _ptr(info)) == _lib.ERR_INVALID_ARG and lib.msbwt_rle_set_walk_piece(None, 64) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, whatever else is wrong with the call; on a loaded index the other guards answer
    # (tests/test_gpu_left_walk.py, test_guards_on_a_loaded_index_in_their_order)
    b = msbwt.RleBWT()
    assert lib.msbwt_rle_walk_info(b._h, None) == _lib.ERR_INVALID_ARG
    for n, max_steps, where in ((2, 4, rows), (2, 4, None), (0, 0, None), (2, 2 ** 40, rows), (2 ** 39, 2, rows)):
        assert lib.msbwt_rle_walk_rows(b._h, None if where is None else _ptr(where), n, max_steps, None, _ptr(steps), None, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_walk_rows_device(b._h, None, n, max_steps, None, None, None, None, None, None) == _lib.ERR_NOT_LOADED
        for out_total in (C.byref(total), None):
            assert lib.msbwt_rle_extract_reads(b._h, None if where is None else _ptr(where), 0, n, max_steps, None, _ptr(steps), 0, out_total,
                                               C.byref(truncated)) == _lib.ERR_NOT_LOADED
            assert lib.msbwt_rle_extract_reads_device(b._h, None, 0, n, max_steps, None, None, 0, out_total, None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (steps == 77).all() and total.value == truncated.value == 99  # refused before anything was written
    for call in (lambda: b.walk_rows(rows, 4), lambda: b.locate_rows(rows, 4), lambda: b.extract_reads(read_ids=[0], max_len=5), lambda: b.extract_reads(n=1, max_len=5)):
        with pytest.raises(msbwt.MsbwtError) as err:
            call()
        assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    with pytest.raises(ValueError):
        b.walk_rows(rows, 4, symbols=np.zeros((2, 5), dtype=np.uint8))
    assert b.walk_info() == dict.fromkeys(("walks", "steps", "dollar", "max_steps", "bad_row", "pieces", "scratch_bytes", "us"), 0)
    b.set_walk_piece(64)
    b.set_walk_piece(2 ** 28)
    b.set_walk_piece(0)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.set_walk_piece(2 ** 28 + 1)
    assert err.value.code == _lib.ERR_INVALID_ARG and "2^28" in str(err.value)


def pad(x):
    return (x + 255) // 256 * 256


def test_plan_is_the_stated_terms():
    plan = msbwt.walk_plan
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 78, 200, 10 ** 6, 2 ** 20, 2 ** 20 + 1, 10 ** 7):
        for max_steps in (0, 1, 7, 8, 9, 100, 2000):
            for piece in (0, 1, 64, 10 ** 5, 2 ** 21, 2 ** 28):
                P = min(n, piece if piece else 2 ** 20)
                assert plan(n, max_steps, host=False, piece=piece) == plan(n, max_steps, symbols=False, host=False, piece=piece) == 256
                locate = 256 + 4 * pad(8 * P) + pad(P)
                assert plan(n, max_steps, symbols=False, piece=piece) == locate, (n, max_steps, piece)
                assert plan(n, max_steps, piece=piece) == locate + pad(P * max_steps), (n, max_steps, piece)
    assert plan(0, 100) == plan(0, 0, False, False, 64) == 0  # a call of no walks allocates nothing
    assert plan(10 ** 9, 100) == plan(2 ** 20, 100)  # the scratch does not grow with n beyond a piece


def test_plan_refuses_what_is_too_large():
    lib = _lib.lib()
    size = C.c_uint64(5)
    for n, max_steps in ((1, 2 ** 40), (0, 2 ** 40), (2 ** 20, 2 ** 20), (2 ** 39 + 1, 2), (3, 2 ** 39), (2 ** 64 - 1, 1), (2 ** 40, 1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.walk_plan(n, max_steps)
        assert err.value.code == _lib.ERR_TOO_LARGE, (n, max_steps)
    for n, max_steps in ((2 ** 20 - 1, 2 ** 20), (2 ** 40 - 1, 1), (1, 2 ** 40 - 1), (2 ** 50, 0)):
        assert lib.msbwt_walk_plan(n, max_steps, 1, 0, 0, C.byref(size)) == 0, (n, max_steps)
    assert size.value == 256
    assert lib.msbwt_walk_plan(10, 10, 1, 1, 0, None) == 0  # the output is optional
    assert lib.msbwt_walk_plan(10, 10, 1, 1, 2 ** 28 + 1, C.byref(size)) == _lib.ERR_INVALID_ARG and size.value == 256


def test_walk_sequences_on_hand_written_arrays():
    seq = msbwt.walk_sequences
    symbols = np.array([[3, 2, 1, 0xEE], [0xEE] * 4, [5, 3, 2, 2]], dtype=np.uint8)  # GTN$$ACCC$G: the walks from rows 0, 3 and 1
    steps = np.array([3, 0, 4], dtype=U64)
    assert seq(symbols, steps, text=True) == ["ACG", "", "CCGT"]
    codes = seq(symbols, steps)
    assert [c.tolist() for c in codes] == [[1, 2, 3], [], [2, 2, 3, 5]] and all(c.dtype == np.uint8 for c in codes)
    assert seq(np.zeros((0, 4), dtype=np.uint8), np.zeros(0, dtype=U64), text=True) == []
    assert seq(np.zeros((2, 0), dtype=np.uint8), np.zeros(2, dtype=U64), text=True) == ["", ""]
    for bad in (dict(steps=np.array([3, 0, 5], dtype=U64)), dict(steps=steps[:2]), dict(symbols=symbols[:2]), dict(symbols=symbols[0])):
        with pytest.raises(ValueError):
            seq(**{**dict(symbols=symbols, steps=steps), **bad})


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "extract_reads")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "extract_reads.c"), "-o", exe] + _link_flags())
    for args in ([], ["--first", "3"], ["index.npy", "--first"], ["index.npy", "--count", "x"], ["index.npy", "--max-len", "0"], ["index.npy", "--width", "5"],
                 ["index.npy", "--piece", "0"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, args


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    exe = str(tmp_path / "left_walk_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "left_walk_mirror.cpp"),
                           "-o", exe] + _link_flags())
    assert subprocess.run([exe]).returncode == 0


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in NEW:
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn walk_rows(&self", "pub fn locate_rows(&self", "pub unsafe fn walk_rows_device(&self", "pub fn extract_reads(&self",
                       "pub unsafe fn extract_reads_device(&self", "pub fn walk_info(&self", "pub fn set_walk_piece(&mut self", "pub fn walk_plan("):
            assert method in text
