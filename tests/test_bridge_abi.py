"""The bridge entry points (include/msbwt_hip.h, "bridges": msbwt_rle_bridge_kmers[_device], msbwt_rle_bridge_info,
msbwt_rle_set_bridge_slots, msbwt_bridge_plan) without a GPU: the symbols and their signatures, the header section's place, the words
of its definition and its constants, the guards that answer before a device is touched, the pure size plan against the terms the
header states and against the layout the call carves, bridge_sequences on hand-written arrays, the example, the C++ mirror and the
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
NEW = ("msbwt_rle_bridge_kmers", "msbwt_rle_bridge_kmers_device", "msbwt_rle_bridge_info", "msbwt_rle_set_bridge_slots", "msbwt_bridge_plan")
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
    assert [len(decls[name][1]) for name in NEW] == [19, 20, 2, 2, 7]
    # the device form: the host form's scalars in their places, every array a device pointer, and the stream
    host, device = decls[NEW[0]][1], decls[NEW[1]][1]
    assert device[-1] == "void *" and [shim.norm_c(t) for t in device[3:12]] == [shim.norm_c(t) for t in host[3:12]]
    assert all(shim.norm_c(t) in ("void *", "const void *") for t in device[1:3] + device[12:])


def test_header_section():
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own behind the read overlaps, before "several GPUs"
    assert header.index("---- read overlaps ----") < header.index("msbwt_overlap_plan(uint64_t") < header.index("---- bridges ----")
    assert header.index("---- bridges ----") < header.index("msbwt_rle_bridge_kmers(") < header.index("msbwt_bridge_plan(uint64_t") < header.index("---- several GPUs")
    section = header[header.index("---- bridges ----"):header.index("---- several GPUs")]
    prose = " ".join(line.strip().lstrip("*").strip() for line in section.splitlines())  # the comment's lines joined: a phrase may wrap
    for phrase in ("G(k, m, me)", "1 <= k <= 31", "A WALK may repeat nodes, the seed included", "lo = max(min_steps, 1)", "stop NO_SEED", "stop NO_TARGET",
                   "found = 0 and depth = 0", "W(0) = {the empty walk standing on s}", "max_steps == 0: stop MAX_STEPS with depth 0", "A < C < G < T",
                   "lexicographic order", "whose new node equals t, when r >= lo", "those numbered below max_paths are written", "W(r) = E(r) \\ B(r)",
                   "An entry into t with r < lo does not end the walk", "found >= max_paths: FULL", "W(r) is empty: EXHAUSTED", "r == max_steps: MAX_STEPS",
                   "|W(r)| > max_live: TOO_WIDE", "ARE ALL COUNTED IN out_found[i]", "(length, then symbols)", "no longer bridge exists", "COUNTING call",
                   "is left untouched", "unused entries are written 0", "0 is never written", "msbwt_rle_device_status", "NULL targets with n > 0", "max_paths == 0",
                   "max_live == 0", "min_steps > max_steps", "MSBWT_ERR_TOO_LARGE", "2^40", "every stop is NO_SEED", "no knob, no index form and no piece size",
                   "the same from run to run", "64 + 8 ceil(max_steps / 32) bytes", "64-bit atomic adds", "STABLE exclusive scan", "once a round", "2^20", "2^28",
                   "6 a pair in round 0, then 4 a state", "msbwt_rle_device_bytes unchanged", "EXACTLY", "pad(P max_paths max_steps)", "DESIGN.md",
                   "the strand-merged graph", "k from 32 on", "edit distance", "per-source thresholds", "several GPUs"):
        assert phrase in prose, phrase
    assert "uint32_t" not in section and "MSBWT_WALK_" not in section
    assert not [line for line in section.splitlines() if line.startswith("#define ")] and "#ifndef MSBWT_BRIDGE_INFO_WORDS" in section
    values = dict(line.split()[2:4] for line in section.splitlines() if line.startswith("#  define MSBWT_BRIDGE_"))
    assert values == {"MSBWT_BRIDGE_RIGHT": "0", "MSBWT_BRIDGE_LEFT": "1", "MSBWT_BRIDGE_EXHAUSTED": "1", "MSBWT_BRIDGE_FULL": "2", "MSBWT_BRIDGE_MAX_STEPS": "3",
                      "MSBWT_BRIDGE_TOO_WIDE": "4", "MSBWT_BRIDGE_NO_SEED": "5", "MSBWT_BRIDGE_NO_TARGET": "6", "MSBWT_BRIDGE_MAX_STEPS_CAP": "4096",
                      "MSBWT_BRIDGE_MAX_LIVE_CAP": "16777216", "MSBWT_BRIDGE_INFO_WORDS": "8"}
    assert _lib.BRIDGE_INFO_WORDS == 8 and _lib.BRIDGE_STOPS == ("", "EXHAUSTED", "FULL", "MAX_STEPS", "TOO_WIDE", "NO_SEED", "NO_TARGET")
    assert _lib.BRIDGE_MAX_STEPS_CAP == 4096 >= 1024 and _lib.BRIDGE_MAX_LIVE_CAP == 16777216
    # the traces no longer call it out of scope, there and in DESIGN.md, and point here
    traces = header[header.index("---- traces ----"):header.index("---- canonical traces ----")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "branching exploration" not in header and "branching exploration" not in design and '"bridges" section' in traces and '"Bridges" below' in design
    assert "### Bridges (" in design


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    words, found = np.array([5, 6], dtype=U64), np.full(2, 77, dtype=U64)
    info = np.full(8, 9, dtype=U64)
    # a null handle
    assert lib.msbwt_rle_bridge_kmers(None, _ptr(words), _ptr(words), 3, 2, 1, 0, 0, 0, 4, 2, 8, None, None, None, _ptr(found), None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_bridge_kmers_device(None, None, None, 3, 0, 1, 0, 0, 0, 4, 2, 8, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_bridge_info(None, _ptr(info)) == _lib.ERR_INVALID_ARG and lib.msbwt_rle_set_bridge_slots(None, 64) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, as everywhere in the API, whatever else is wrong with the call; on a loaded index the
    # other guards answer (tests/test_gpu_bridges.py)
    b = msbwt.RleBWT()
    assert lib.msbwt_rle_bridge_info(b._h, None) == _lib.ERR_INVALID_ARG
    for k in (0, 3, 31, 32):
        for min_count, min_edge in ((1, 0), (3, 2)):
            for direction, n, min_steps, max_steps, max_paths, max_live in ((0, 2, 0, 4, 2, 8), (2, 2, 0, 4, 2, 8), (0, 2, 5, 4, 2, 8), (0, 2, 0, 4, 0, 8), (0, 2, 0, 4, 2, 0),
                                                                           (0, 2, 0, 5000, 2, 8), (0, 2, 0, 4, 2, 2 ** 25), (0, 2 ** 30, 0, 2 ** 5, 2 ** 5, 8), (0, 0, 0, 0, 1, 1)):
                assert lib.msbwt_rle_bridge_kmers(b._h, _ptr(words), _ptr(words), k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, None, None,
                                                  None, _ptr(found), None, None, None) == _lib.ERR_NOT_LOADED
                assert lib.msbwt_rle_bridge_kmers_device(b._h, None, None, k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, None, None, None,
                                                         None, None, None, None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (found == 77).all()  # refused before anything was written
    with pytest.raises(msbwt.MsbwtError) as err:
        b.bridge_kmers(words, words, 3, 4, direction="left")
    assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    with pytest.raises(KeyError):
        b.bridge_kmers(words, words, 3, 4, direction="up")
    with pytest.raises(ValueError):
        b.bridge_kmers(words, words[:1], 3, 4)
    with pytest.raises(ValueError):
        b.bridge_kmers(words, words, 3, 4, symbols=np.zeros((2, 4, 5), dtype=np.uint8))
    assert b.bridge_info() == dict.fromkeys(("pairs", "rounds", "queries", "expanded", "found", "pieces", "scratch_bytes", "widest"), 0)
    b.set_bridge_slots(64)
    b.set_bridge_slots(2 ** 28)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.set_bridge_slots(2 ** 28 + 1)
    assert err.value.code == _lib.ERR_INVALID_ARG and "2^28" in str(err.value)
    b.set_bridge_slots(0)


def pad(x):
    return (x + 255) // 256 * 256


def scan_words(x):
    w = 1
    while x > 2048:
        x = -(-x // 2048)
        w += x
    return w


def test_plan_is_the_stated_terms():
    plan = msbwt.bridge_plan
    for n in (1, 2, 31, 64, 65, 200, 2 ** 14, 2 ** 14 + 1, 10 ** 6):
        for max_steps in (0, 1, 32, 33, 100, 4096):
            for max_paths in (1, 4):
                for max_live in (1, 3, 64, 2 ** 16, 2 ** 21):
                    for slots in (0, 1, 64, 10 ** 5, 2 ** 22):
                        s = max(slots or 2 ** 20, max_live)
                        P = min(n, s // max_live)
                        S, W = P * max_live, 8 + -(-max_steps // 32)
                        terms = [256, pad(48 * P), 2 * pad(8 * W * S), pad(8 * S), pad(8 * scan_words(S)), 2 * pad(8 * max(4 * S, 6 * P))]
                        assert plan(n, max_steps, max_paths, max_live, host=False, slots=slots) == sum(terms), (n, max_steps, max_paths, max_live, slots)
                        staged = [2 * pad(8 * P), pad(P * max_paths * max_steps), 2 * pad(8 * P * max_paths), 3 * pad(8 * P) + pad(P)]
                        assert plan(n, max_steps, max_paths, max_live, slots=slots) == sum(terms) + sum(staged), (n, max_steps, max_paths, max_live, slots)
    assert plan(0, 100) == plan(0, 0, 1, 1, False, 64) == 0  # a call of no pairs allocates nothing
    assert plan(10 ** 9, 100, host=False) == plan(2 ** 14, 100, host=False)  # the scratch does not grow with n beyond a piece
    assert plan(5, 100, max_live=64, slots=7, host=False) == plan(1, 100, max_live=64, host=False)  # max_live above the slots: a pair a piece


def test_plan_refuses_what_is_too_large():
    lib = _lib.lib()
    size = C.c_uint64(5)
    for n, max_steps, max_paths, max_live in ((1, 4097, 1, 1), (0, 4097, 1, 1), (1, 10, 1, 2 ** 24 + 1), (2 ** 30, 2 ** 5, 2 ** 5, 8), (2 ** 28, 4096, 1, 1), (2, 0, 2 ** 39, 1),
                                              (1, 0, 2 ** 40, 1), (2 ** 64 - 1, 1, 1, 1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.bridge_plan(n, max_steps, max_paths, max_live)
        assert err.value.code == _lib.ERR_TOO_LARGE, (n, max_steps, max_paths, max_live)
    for n, max_steps, max_paths, max_live in ((2 ** 28 - 1, 4096, 1, 1), (2 ** 40 - 1, 1, 1, 1), (1, 4096, 2 ** 28 - 1, 2 ** 24), (2 ** 20, 0, 2 ** 19, 1)):
        assert lib.msbwt_bridge_plan(n, max_steps, max_paths, max_live, 0, 0, C.byref(size)) == 0, (n, max_steps, max_paths, max_live)
    assert lib.msbwt_bridge_plan(10, 10, 4, 64, 1, 0, None) == 0  # the output is optional
    for max_paths, max_live, slots in ((0, 64, 0), (4, 0, 0), (4, 64, 2 ** 28 + 1)):
        assert lib.msbwt_bridge_plan(10, 10, max_paths, max_live, 1, slots, C.byref(size)) == _lib.ERR_INVALID_ARG


def test_bridge_sequences_on_hand_written_arrays():
    seq = msbwt.bridge_sequences
    k = 3
    seeds = np.array([0b000110, 0b111111 | 1 << 40, 0b100100], dtype=U64)  # ACG, TTT with garbage above bit 2k, GCA
    symbols = np.array([[[1, 5, 0xEE, 0xEE], [2, 2, 3, 5]], [[0xEE] * 4, [0xEE] * 4], [[3, 0xEE, 0xEE, 0xEE], [0xEE] * 4]], dtype=np.uint8)
    lengths = np.array([[2, 4], [0, 0], [1, 0]], dtype=U64)
    assert seq(seeds, k, symbols, lengths, text=True) == [["ACGAT", "ACGCCGT"], [], ["GCAG"]]
    assert seq(seeds, k, symbols, lengths, "left", text=True) == [["TAACG", "TGCCACG"], [], ["GGCA"]]
    codes = seq(seeds, k, symbols, lengths)
    assert [[c.tolist() for c in rows] for rows in codes] == [[[1, 2, 3, 1, 5], [1, 2, 3, 2, 2, 3, 5]], [], [[3, 2, 1, 3]]]
    assert all(c.dtype == np.uint8 for rows in codes for c in rows)
    assert seq(np.zeros(0, dtype=U64), k, np.zeros((0, 2, 4), dtype=np.uint8), np.zeros((0, 2), dtype=U64), text=True) == []
    for bad in (dict(lengths=np.array([[2, 5], [0, 0], [1, 0]], dtype=U64)), dict(lengths=lengths[:2]), dict(symbols=symbols[:2]), dict(symbols=symbols[:, 0]),
                dict(direction="up")):
        with pytest.raises(ValueError):
            seq(seeds, k, **{**dict(symbols=symbols, lengths=lengths), **bad})


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "bridge_kmers")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "bridge_kmers.c"), "-o", exe] + _link_flags())
    for args in ([], ["5"], ["5", "2"], ["0", "2", "ACGTACGT"], ["32", "2", "ACGTACGT"], ["5", "0", "ACGTACGT"], ["x", "2", "ACGTACGT"], ["5", "2x", "ACGTACGT"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_program_compiles_and_runs(tmp_path):
    exe = str(tmp_path / "bridges_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bridges_mirror.cpp"),
                           "-o", exe] + _link_flags())
    assert subprocess.run([exe]).returncode == 0


def test_layout_matches_the_plan_term_by_term(tmp_path):
    """the offsets the call carves (graph_layouts.hpp) are the running sums of the plan's terms, in the header's order"""
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include "graph_layouts.hpp"\n'
                   "int main() {\n"
                   "    const msbwt::BridgeLayout l = msbwt::bridge_layout(8, 40, 3, 8, true, 1);\n"
                   '    std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\\n", (unsigned long long)l.counters,\n'
                   "                (unsigned long long)l.table, (unsigned long long)l.states[0], (unsigned long long)l.states[1], (unsigned long long)l.weights,\n"
                   "                (unsigned long long)l.scan, (unsigned long long)l.queries, (unsigned long long)l.counts, (unsigned long long)l.seeds,\n"
                   "                (unsigned long long)l.targets, (unsigned long long)l.symbols, (unsigned long long)l.lengths, (unsigned long long)l.edge_sums,\n"
                   "                (unsigned long long)l.found, (unsigned long long)l.stops, (unsigned long long)l.depths, (unsigned long long)l.live, (unsigned long long)l.bytes);\n"
                   "    return msbwt::bridge_piece_pairs(200, 8, 64) == 8 && msbwt::bridge_piece_pairs(200, 64, 7) == 1 && msbwt::bridge_piece_pairs(3, 8, 0) == 3 ? 0 : 1;\n"
                   "}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(LIBDIR, "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0
    P, S, W = 8, 64, 10
    extents = [256, pad(48 * P), pad(8 * W * S), pad(8 * W * S), pad(8 * S), pad(8), pad(8 * 4 * S), pad(8 * 4 * S), pad(8 * P), pad(8 * P), pad(P * 3 * 40),
               pad(8 * P * 3), pad(8 * P * 3), pad(8 * P), pad(P), pad(8 * P), pad(8 * P)]
    assert [int(x) for x in r.stdout.split()] == [sum(extents[:i]) for i in range(len(extents) + 1)]
    assert sum(extents) == msbwt.bridge_plan(200, 40, 3, 8, host=True, slots=64)


def test_both_shim_copies_declare_the_calls_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in NEW:
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        for method in ("pub fn bridge_kmers(&self", "pub unsafe fn bridge_kmers_device(&self", "pub fn bridge_info(&self", "pub fn set_bridge_slots(&mut self",
                       "pub fn bridge_plan("):
            assert method in text
