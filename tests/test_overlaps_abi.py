"""The read-overlap entry points (include/msbwt_hip.h, "read overlaps": msbwt_rle_read_overlaps[_device], msbwt_rle_overlap_info,
msbwt_rle_set_overlap_piece, msbwt_overlap_plan) without a GPU: the symbols and their signatures, the header section's place, the
phrases of its definitions and its constants, the guards that answer before a device is touched, the pure size plan against the
terms the header states, overlap_edges on hand-written records, the example, the C++ mirror and the shim's two copies."""
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
NEW = ("msbwt_rle_read_overlaps", "msbwt_rle_read_overlaps_device", "msbwt_rle_overlap_info", "msbwt_rle_set_overlap_piece", "msbwt_overlap_plan")
U64 = np.uint64


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p,
                "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "const uint64_t *": C.c_void_p, "uint8_t *": C.c_void_p, "const uint8_t *": C.c_void_p,
                "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int": C.c_int}
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
    assert [len(decls[name][1]) for name in NEW] == [16, 17, 2, 2, 6]
    # the device form: the host form's arguments as device pointers, out_record_total a host pointer, and the stream
    host, device = decls[NEW[0]][1], decls[NEW[1]][1]
    assert device[-1] == "void *" and [shim.norm_c(t) for t in device[3:7]] == [shim.norm_c(t) for t in host[3:7]] and shim.norm_c(device[12]) == "uint64_t *"


def test_header_section():
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own behind the left walks, before "several GPUs"
    assert header.index("---- left walks ----") < header.index("msbwt_walk_plan(uint64_t") < header.index("---- read overlaps ----")
    assert header.index("---- read overlaps ----") < header.index("msbwt_rle_read_overlaps(") < header.index("msbwt_overlap_plan(uint64_t") < header.index("---- several GPUs")
    section = header[header.index("---- read overlaps ----"):header.index("---- several GPUs")]
    prose = " ".join(line.strip().lstrip("*").strip() for line in section.splitlines())  # the comment's lines joined: a phrase may wrap
    for phrase in ("on the BWT string alone", "any loaded stream", "constrain(c, [l, h)) = [C[c] + rank(c, l), C[c] + rank(c, h))", "L >= 0 symbol codes",
                   "min_overlap = m >= 1", "max_overlap = M (0 means no limit)", "COMPLEMENT_INT = [0,5,3,2,4,1]", "N stays N", "E = min(L, M)", "R_0 = [0, T)",
                   "If j >= m and D_j = [rank('$', l_j), rank('$', h_j)) is not empty, emit the record (j, D_j.l, D_j.h - D_j.l)", "If j == E, stop END",
                   "c = Q'[L - 1 - j]", "If c is 0 or above 5, stop BAD_SYMBOL", "The records emitted so far stand", "R_(j+1) = constrain(c, R_j)",
                   "If it is empty, stop EMPTY", "in ascending j", "the longest suffix of Q', up to E symbols, that occurs in the index",
                   "the sum of the counts of its records", "every read that contains Q as a prefix", "is the caller's policy", "they need no alignment",
                   "always set, NULL is MSBWT_ERR_INVALID_ARG", "COUNTING call", "TWO searches", "the message names R", "unspecified within their capacity",
                   "nothing is written past it", "MSBWT_ERR_INVALID_SYMBOL", "msbwt_rle_device_status", "0 is never written", "in this order", "no BWT loaded",
                   "min_overlap == 0", "only some of the three columns", "MSBWT_ERR_INVALID_RANGE", "MSBWT_ERR_TOO_LARGE", "2^40", "out_offsets[0] = 0",
                   "nothing is allocated", "no knob, no index form and no piece", "ONE line when both bounds lie in the same block", "Step 0 needs no line",
                   "2 matched + 2 lines", "OVERFLOW run block", "2^20", "2^28", "msbwt_rle_device_bytes unchanged", "EXACTLY", "pad(piece_symbols)",
                   "3 pad(8 piece_records)", "DESIGN.md", "msbwt_rle_extract_reads", "several GPUs", "Pair blocks and the direct and sparse tables are left out"):
        assert phrase in prose, phrase
    assert "uint32_t" not in section
    assert not [line for line in section.splitlines() if line.startswith("#define ")] and "MSBWT_WALK_" not in section.split("---- read overlaps ----")[1].split("#ifndef")[1]
    values = dict(line.split()[2:4] for line in section.splitlines() if line.startswith("#  define MSBWT_OVERLAP_"))
    assert values == {"MSBWT_OVERLAP_END": "1", "MSBWT_OVERLAP_EMPTY": "2", "MSBWT_OVERLAP_BAD_SYMBOL": "3", "MSBWT_OVERLAP_INFO_WORDS": "13"}
    assert _lib.OVERLAP_INFO_WORDS == 13 and _lib.OVERLAP_STOPS == ("", "END", "EMPTY", "BAD_SYMBOL")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    flat, offsets = np.array([1, 2, 3, 5], dtype=np.uint8), np.array([0, 2, 4], dtype=U64)
    out = np.full(8, 77, dtype=U64)
    info = np.full(13, 9, dtype=U64)
    total = C.c_uint64(99)
    # a null handle
    assert lib.msbwt_rle_read_overlaps(None, _ptr(flat), _ptr(offsets), 2, 1, 0, 0, _ptr(out), None, None, None, 0, C.byref(total), None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_read_overlaps_device(None, None, None, 0, 1, 0, 0, None, None, None, None, 0, C.byref(total), None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_overlap_info(None, _ptr(info)) == _lib.ERR_INVALID_ARG and lib.msbwt_rle_set_overlap_piece(None, 64) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, whatever else is wrong with the call; on a loaded index the other guards answer
    # (tests/test_gpu_overlaps.py, test_guards_on_a_loaded_index_in_their_order)
    b = msbwt.RleBWT()
    assert lib.msbwt_rle_overlap_info(b._h, None) == _lib.ERR_INVALID_ARG
    decreasing = np.array([0, 4, 2], dtype=U64)
    for n, m, strand, where, offs, out_total, columns in ((2, 1, 0, flat, offsets, True, 0), (2, 0, 0, flat, offsets, True, 0), (2, 1, 2, flat, offsets, True, 0),
                                                          (2, 1, 0, None, offsets, True, 0), (2, 1, 0, flat, None, True, 0), (2, 1, 0, flat, offsets, False, 0),
                                                          (2, 1, 0, flat, offsets, True, 1), (2, 1, 0, flat, offsets, True, 2), (2 ** 40, 1, 0, flat, offsets, True, 0),
                                                          (2, 1, 0, flat, decreasing, True, 0), (0, 1, 0, None, None, True, 0)):
        cols = [_ptr(out) if i < columns else None for i in range(3)]
        where_total = C.byref(total) if out_total else None
        assert lib.msbwt_rle_read_overlaps(b._h, None if where is None else _ptr(where), None if offs is None else _ptr(offs), n, m, 0, strand, _ptr(out), *cols, 8,
                                           where_total, None, None, None) == _lib.ERR_NOT_LOADED
        assert lib.msbwt_rle_read_overlaps_device(b._h, None, None, n, m, 0, strand, None, *cols, 8, where_total, None, None, None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (out == 77).all() and total.value == 99  # refused before anything was written
    for call in (lambda: b.read_overlaps([flat], 1), lambda: b.read_overlaps(["ACGT"], 1, ascii=True, records=False), lambda: b.read_overlaps((flat, offsets), 3, strand=1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            call()
        assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    assert b.overlap_info() == dict.fromkeys(("queries", "symbols", "records", "edges", "end", "empty", "bad_symbol", "lines", "pieces", "scratch_bytes", "us", "piece_symbols",
                                              "piece_records"), 0)
    # the piece's limits
    b.set_overlap_piece(64)
    b.set_overlap_piece(2 ** 28)
    b.set_overlap_piece(0)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.set_overlap_piece(2 ** 28 + 1)
    assert err.value.code == _lib.ERR_INVALID_ARG and "2^28" in str(err.value)


def pad(x):
    return (x + 255) // 256 * 256


def stated_plan(n, host, piece, piece_symbols, piece_records):
    """the terms include/msbwt_hip.h states"""
    if n == 0:
        return 0
    P = min(n, piece if piece else 2 ** 20)
    w, x = 1, P + 1
    while x > 2048:
        x = -(-x // 2048)
        w += x
    size = 256 + pad(8 * (P + 1)) + pad(8 * w)
    if host:
        size += 2 * pad(8 * (P + 1)) + 2 * pad(8 * P) + pad(P) + pad(piece_symbols) + (3 * pad(8 * piece_records) if piece_records else 0)
    return size


def test_plan_is_the_stated_terms():
    plan = msbwt.overlap_plan
    for n in (0, 1, 2, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 10 ** 6, 2 ** 20, 2 ** 20 + 1, 10 ** 7):
        for piece in (0, 1, 64, 2047, 2048, 10 ** 5, 2 ** 21, 2 ** 22 + 5, 2 ** 28):
            for piece_symbols, piece_records in ((0, 0), (1, 1), (255, 31), (256, 32), (257, 33), (10 ** 6, 123457)):
                for host in (False, True):
                    assert plan(n, host, piece, piece_symbols, piece_records) == stated_plan(n, host, piece, piece_symbols, piece_records), (n, host, piece, piece_symbols)
    assert plan(10 ** 9, False) == plan(2 ** 20, False) and plan(10 ** 9, True, 0, 5000, 70) == plan(2 ** 20, True, 0, 5000, 70)  # no growth beyond a piece
    assert plan(100, False, 0, 10 ** 6, 10 ** 6) == plan(100, False)  # the device form stages nothing


def test_plan_refuses_what_is_too_large():
    lib = _lib.lib()
    size = C.c_uint64(5)
    for n, symbols, records in ((2 ** 40, 0, 0), (2 ** 64 - 1, 0, 0), (5, 2 ** 40, 0), (5, 0, 2 ** 40)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.overlap_plan(n, True, 0, symbols, records)
        assert err.value.code == _lib.ERR_TOO_LARGE, (n, symbols, records)
    assert lib.msbwt_overlap_plan(2 ** 40 - 1, 0, 1, 0, 0, C.byref(size)) == 0 and size.value == 256 + 256 + 256
    assert lib.msbwt_overlap_plan(10, 1, 0, 10, 10, None) == 0  # the output is optional
    assert lib.msbwt_overlap_plan(10, 1, 2 ** 28 + 1, 0, 0, C.byref(size)) == _lib.ERR_INVALID_ARG and size.value == 768


class _Result:
    pass


def test_overlap_edges_on_hand_written_records():
    r = _Result()
    # query 0 (length 4): reads 3, 4 at length 2 and read 1 at length 4; query 1 (length 2): nothing; query 2 (length 3): reads 0, 1, 2 at length 3
    r.offsets, r.lengths, r.first, r.counts = np.array([0, 2, 2, 3], dtype=U64), np.array([2, 4, 3], dtype=U64), np.array([3, 1, 0], dtype=U64), np.array([2, 1, 3], dtype=U64)
    r.query_lengths = np.array([4, 2, 3], dtype=U64)
    every = [[0, 3, 2], [0, 4, 2], [0, 1, 4], [2, 0, 3], [2, 1, 3], [2, 2, 3]]
    edges = msbwt.overlap_edges(r)
    assert edges.dtype == U64 and edges.tolist() == every
    assert msbwt.overlap_edges(r, query_ids=[1, 9, 2]).tolist() == [e for e in every if e not in ([0, 1, 4], [2, 2, 3])]
    assert msbwt.overlap_edges(r, query_ids=[1, 9, 2], drop_self=False).tolist() == every
    assert msbwt.overlap_edges(r, query_ids=[0, 0, 0]).tolist() == [e for e in every if e != [2, 0, 3]]
    assert msbwt.overlap_edges(r, drop_contained=True).tolist() == every[:2]
    assert msbwt.overlap_edges(r, query_ids=[1, 9, 2], drop_contained=True).tolist() == every[:2]
    r.lengths = None
    with pytest.raises(ValueError):
        msbwt.overlap_edges(r)
    empty = msbwt.OverlapResult(0, np.zeros(0, dtype=U64))
    empty.lengths = empty.first = empty.counts = np.zeros(0, dtype=U64)
    assert msbwt.overlap_edges(empty).shape == (0, 3)


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "read_overlaps")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "read_overlaps.c"), "-o", exe] + _link_flags())
    for args in ([], ["--min-overlap", "3"], ["index.npy", "--min-overlap"], ["index.npy", "--min-overlap", "x"], ["index.npy", "--min-overlap", "0"],
                 ["index.npy", "--max-len", "0"], ["index.npy", "--width", "5"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, args


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    exe = str(tmp_path / "overlaps_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "overlaps_mirror.cpp"),
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
        for method in ("pub fn read_overlaps(&self", "pub unsafe fn read_overlaps_device(&self", "pub fn overlap_info(&self", "pub fn set_overlap_piece(&mut self",
                       "pub fn overlap_plan("):
            assert method in text
