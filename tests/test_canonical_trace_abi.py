"""The canonical trace entry points (include/msbwt_hip.h, "canonical traces": msbwt_rle_trace_canonical_kmers[_device],
msbwt_rle_canonical_trace_info, msbwt_canonical_trace_plan) without a GPU: the symbols and their signatures, the guards that answer
before a device is touched, the pure size plan against the terms the header states, the header section's key words and its two defines,
the example, the C++ mirror and the shim's two copies."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_trace_abi import _link_flags, _ptr, pad

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
NEW = ("msbwt_rle_trace_canonical_kmers", "msbwt_rle_trace_canonical_kmers_device", "msbwt_rle_canonical_trace_info", "msbwt_canonical_trace_plan")
TWIN = {"msbwt_rle_trace_canonical_kmers": "msbwt_rle_trace_kmers", "msbwt_rle_trace_canonical_kmers_device": "msbwt_rle_trace_kmers_device",
        "msbwt_rle_canonical_trace_info": "msbwt_rle_trace_info", "msbwt_canonical_trace_plan": "msbwt_trace_plan"}
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
        # the parameter list of the trace call it stands beside, type for type
        assert [shim.norm_c(ct) for ct in cparams] == [shim.norm_c(ct) for ct in decls[TWIN[name]][1]] and shim.norm_c(cret) == shim.norm_c(decls[TWIN[name]][0]), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[TWIN[name]]
    assert len(decls["msbwt_rle_trace_canonical_kmers"][1]) == 16 and len(decls["msbwt_rle_trace_canonical_kmers_device"][1]) == 17


def test_header_section():
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own directly behind the traces
    assert header.index("---- traces ----") < header.index("msbwt_trace_plan(uint64_t") < header.index("---- canonical traces ----")
    assert header.index("---- canonical traces ----") < header.index("msbwt_rle_trace_canonical_kmers(") < header.index("---- several GPUs")
    traces = header[header.index("---- traces ----"):header.index("---- canonical traces ----")]
    assert '"canonical traces"' in traces and "per-source" in traces  # the traces' "out of scope" points here
    section = header[header.index("---- canonical traces ----"):header.index("---- several GPUs")]
    for word in ("D(k, m, me)", '"canonical unitigs"', "cc(x) = count_kmer(x) + count_kmer(rc(x))", "palindrome", "AND q' is a node", '{"CATG"}', "FAN", "BACK-FAN",
                 "3b.", "MSBWT_CANONICAL_TRACE_MIRROR", "BEFORE 4", "MIRROR, not MERGE", "largest cc", "smallest symbol", "edge_sum += cc(e)", "hairpin",
                 "stated, not cured", "msbwt_rle_enumerate_canonical_unitigs", "out_ends >> 4", "out_ends & 15", "1 <= k <= 31", "(10 + E) n", "16 + 2 E",
                 "msbwt_rle_device_status", "msbwt_rle_set_trace_piece governs both", "w = 18", "else 11", "EXACTLY", "DESIGN.md", "NOT_A_NODE", "RETURNED"):
        assert word in section, word
    assert "uint32_t" not in section
    values = dict(line.split()[1:3] for line in section.splitlines() if line.startswith("#define "))
    assert values == {"MSBWT_CANONICAL_TRACE_MIRROR": "8", "MSBWT_CANONICAL_TRACE_INFO_WORDS": "8"}
    assert _lib.CANONICAL_TRACE_INFO_WORDS == 8 and _lib.CANONICAL_TRACE_STOPS[:8] == _lib.TRACE_STOPS and _lib.CANONICAL_TRACE_STOPS[8:] == ("MIRROR",)
    assert len(_lib.TRACE_STOPS) == 8


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    seeds, steps = np.array([5, 6], dtype=U64), np.full(2, 77, dtype=U64)
    info = np.full(8, 9, dtype=U64)
    # a null handle
    assert lib.msbwt_rle_trace_canonical_kmers(None, _ptr(seeds), None, 3, 2, 1, 0, 0, 0, 4, None, _ptr(steps), None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_trace_canonical_kmers_device(None, None, None, 3, 0, 1, 0, 0, 0, 4, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_canonical_trace_info(None, _ptr(info)) == _lib.ERR_INVALID_ARG and (info == 9).all()
    # nothing loaded: the index is checked first, as everywhere in the API, whatever else is wrong with the call; on a loaded index the
    # other guards answer (tests/test_gpu_canonical_trace.py)
    b = msbwt.RleBWT()
    assert lib.msbwt_rle_canonical_trace_info(b._h, None) == _lib.ERR_INVALID_ARG
    for k in (0, 3, 31, 32, 33):
        for min_count, min_edge in ((1, 0), (3, 2)):
            for mode, direction, n, max_steps in ((0, 0, 2, 4), (3, 0, 2, 4), (0, 2, 2, 4), (0, 0, 2, 2 ** 40), (0, 0, 0, 0)):
                assert lib.msbwt_rle_trace_canonical_kmers(b._h, _ptr(seeds), None, k, n, min_count, min_edge, mode, direction, max_steps, None, _ptr(steps), None,
                                                           None, None, None) == _lib.ERR_NOT_LOADED
                assert lib.msbwt_rle_trace_canonical_kmers_device(b._h, None, None, k, n, min_count, min_edge, mode, direction, max_steps, None, None, None, None, None,
                                                                  None, None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (steps == 77).all()  # refused before anything was written
    with pytest.raises(msbwt.MsbwtError) as err:
        b.trace_canonical_kmers(seeds, 3, 4, mode="unitig", direction="left")
    assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    with pytest.raises(KeyError):
        b.trace_canonical_kmers(seeds, 3, 4, mode="shortest")
    with pytest.raises(KeyError):
        b.trace_canonical_kmers(seeds, 3, 4, direction="up")
    zeros = dict.fromkeys(("walks", "rounds", "queries", "steps", "longest", "pieces", "scratch_bytes", "not_nodes"), 0)
    assert b.canonical_trace_info() == zeros and b.trace_info() == zeros


def test_plan_is_the_stated_terms():
    plan = msbwt.canonical_trace_plan
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 200, 10 ** 6, 2 ** 20, 2 ** 20 + 1, 10 ** 7):
        for max_steps in (0, 1, 7, 100, 2000):
            for piece in (0, 1, 64, 10 ** 5, 2 ** 21):
                P = min(n, piece if piece else 2 ** 20)
                for mode in ("unique", "unitig", "greedy"):
                    w = 18 if mode == "unitig" else 11
                    device = 256 + 2 * pad(64 * P) + 2 * pad(8 * w * P)
                    assert plan(n, max_steps, mode, host=False, piece=piece) == plan(n, max_steps, mode, targets=True, host=False, piece=piece) == device
                    host = device + pad(8 * P) + pad(P * max_steps) + 3 * pad(8 * P) + 2 * pad(P)
                    assert plan(n, max_steps, mode, piece=piece) == host, (n, max_steps, piece, mode)
                    assert plan(n, max_steps, mode, targets=True, piece=piece) == host + pad(8 * P)
                    # the trace plan with another w, and nothing else
                    assert plan(n, max_steps, mode, piece=piece) - msbwt.trace_plan(n, max_steps, mode, piece=piece) == 2 * (pad(8 * w * P) - pad(8 * (8 if w == 18 else 5) * P))
    # the sum written out: 64 walks a piece, 64 x 64 bytes a state buffer, 64 x 18 words of queries and as many of counts
    assert plan(200, 7, "unitig", targets=True, host=False, piece=64) == 256 + 2 * 4096 + 2 * 9216
    assert plan(200, 7, "greedy", targets=True, host=False, piece=64) == 256 + 2 * 4096 + 2 * 5632
    assert plan(0, 100) == plan(0, 0, "unitig", True, False, 64) == 0  # a call of no walks allocates nothing
    assert plan(10 ** 9, 100, host=False) == plan(2 ** 20, 100, host=False)  # the scratch does not grow with n beyond a piece
    assert plan(10 ** 4, 10 ** 7 * 10, host=False) == plan(10 ** 4, 1, host=False)  # nor, in the device form, with max_steps


def test_plan_refuses_what_is_too_large_and_a_mode_that_is_none():
    lib = _lib.lib()
    size = C.c_uint64(5)
    for n, max_steps in ((1, 2 ** 40), (0, 2 ** 40), (2 ** 20, 2 ** 20), (2 ** 39 + 1, 2), (3, 2 ** 39), (2 ** 64 - 1, 1), (2 ** 40, 1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.canonical_trace_plan(n, max_steps)
        assert err.value.code == _lib.ERR_TOO_LARGE, (n, max_steps)
    for n, max_steps in ((2 ** 20 - 1, 2 ** 20), (2 ** 40 - 1, 1), (1, 2 ** 40 - 1), (2 ** 50, 0)):
        assert lib.msbwt_canonical_trace_plan(n, max_steps, 0, 0, 0, 0, C.byref(size)) == 0, (n, max_steps)
    assert lib.msbwt_canonical_trace_plan(10, 10, 0, 0, 1, 0, None) == 0  # the output is optional
    for mode in (-1, 3):
        assert lib.msbwt_canonical_trace_plan(10, 10, mode, 0, 1, 0, C.byref(size)) == _lib.ERR_INVALID_ARG


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "trace_canonical_kmers")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "trace_canonical_kmers.c"), "-o", exe] + _link_flags())
    for args in ([], ["5"], ["0", "ACGTACGT"], ["32", "ACGTACGT"], ["x", "ACGTACGT"], ["5x", "ACGTACGT"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    if (msbwt::RleBWT::canonical_trace_plan(200, 7, MSBWT_TRACE_UNITIG, true, false, 64) != 256 + 2 * 4096 + 2 * 9216) return 1;\n"
                   "    if (msbwt::RleBWT::canonical_trace_plan(0, 7) != 0) return 1;\n"
                   "    try { msbwt::RleBWT::canonical_trace_plan(2, std::uint64_t(1) << 40); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    msbwt::RleBWT::Traces (msbwt::RleBWT::*trace)(const std::vector<std::uint64_t> &, std::size_t, std::uint64_t, int, int, std::uint64_t, std::uint64_t,\n"
                   "                                                  const std::vector<std::uint64_t> &) const = &msbwt::RleBWT::trace_canonical_kmers;\n"
                   "    void (msbwt::RleBWT::*device)(const void *, const void *, std::size_t, std::size_t, std::uint64_t, std::uint64_t, int, int, std::uint64_t, void *, void *,\n"
                   "                                  void *, void *, void *, void *, void *) const = &msbwt::RleBWT::trace_canonical_kmers_device;\n"
                   "    msbwt::RleBWT::TraceInfo (msbwt::RleBWT::*info)() const = &msbwt::RleBWT::canonical_trace_info;\n"
                   "    return trace && device && info && MSBWT_CANONICAL_TRACE_MIRROR == 8 && MSBWT_CANONICAL_TRACE_INFO_WORDS == 8 ? 0 : 1;\n"
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
        for method in ("pub fn trace_canonical_kmers(&self", "pub unsafe fn trace_canonical_kmers_device(&self", "pub fn canonical_trace_info(&self",
                       "pub fn canonical_trace_plan("):
            assert method in text
