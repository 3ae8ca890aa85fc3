"""The canonical unitig entry points (include/msbwt_hip.h: msbwt_rle_enumerate_canonical_unitigs[_device],
msbwt_rle_canonical_unitig_info, msbwt_canonical_unitigs_plan) without a GPU: the symbols and their signatures, the guards that answer
before a device is touched, the pure size plan against the formula the header states, the example, the C++ mirror and the shim's two
copies."""
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
NEW = ("msbwt_rle_enumerate_canonical_unitigs", "msbwt_rle_enumerate_canonical_unitigs_device", "msbwt_rle_canonical_unitig_info",
       "msbwt_canonical_unitigs_plan")
INFO = ("classes", "edge_classes", "links", "unitigs", "symbols", "circular", "longest", "rounds", "palindromes", "cut_links")
C4, HUMAN = 1_950_000_000, 90_000_000_000
FREE = 250 * 10 ** 9
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
        # the parameter lists are those of the strand-specific calls
        assert decls[name] == decls[name.replace("canonical_", "")], name
    header = open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()
    # a section of its own, after the unitigs' plan and before the scratch report; the definitions are in it
    assert header.index("msbwt_unitigs_plan(uint64_t") < header.index("---- canonical unitigs ----") < header.index("msbwt_rle_enumerate_canonical_unitigs(")
    assert header.index("msbwt_canonical_unitigs_plan(uint64_t") < header.index("msbwt_rle_spectrum_scratch_bytes(const")
    section = header[header.index("---- canonical unitigs ----"):header.index("msbwt_rle_enumerate_canonical_unitigs(")]
    for word in ("CLASSES", "NODES", "EDGES", "LINKS", "CHOICE", "OUTPUTS", "TOTALS", "S = n + U (k - 1)", "both\n * q and q' are nodes", "CATG", "palindromic node has no links",
                 "k = 32 is MSBWT_ERR_INVALID_ARG", "binary search"):
        assert word in section, word
    # the strand-specific section points here
    plain = header[header.index("---- unitigs ----"):header.index("msbwt_rle_enumerate_unitigs(")]
    assert "out of scope of THIS call: see the canonical unitigs below" in plain
    assert "#define MSBWT_CANONICAL_UNITIG_INFO_WORDS 10" in header and _lib.CANONICAL_UNITIG_INFO_WORDS == 10 == len(INFO)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_guards_answer_without_a_device():
    lib = _lib.lib()
    u, s = C.c_uint64(77), C.c_uint64(78)
    info = np.full(10, 7, dtype=U64)
    bufs = [np.full(4, 7, dtype=t) for t in (np.uint8, U64, U64, np.uint8, np.uint8)]
    ptrs = [_ptr(a) for a in bufs]
    # a null handle
    assert lib.msbwt_rle_enumerate_canonical_unitigs(None, 3, 1, 0, *ptrs, 4, 4, C.byref(u), C.byref(s)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_canonical_unitigs_device(None, 3, 1, 0, None, None, None, None, None, 0, 0, C.byref(u), C.byref(s), None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_canonical_unitig_info(None, _ptr(info)) == _lib.ERR_INVALID_ARG
    # nothing loaded: the index is checked first, as everywhere in the API, so a bad k and a min_edge below the node threshold are
    # MSBWT_ERR_NOT_LOADED here; on a loaded index they are MSBWT_ERR_INVALID_ARG (tests/test_gpu_canonical_unitigs.py)
    b = msbwt.RleBWT()
    for k in (0, 3, 32, 33):
        for min_count, min_edge in ((1, 0), (3, 2), (2, 5)):
            assert lib.msbwt_rle_enumerate_canonical_unitigs(b._h, k, min_count, min_edge, *ptrs, 4, 4, C.byref(u), C.byref(s)) == _lib.ERR_NOT_LOADED
            assert lib.msbwt_rle_enumerate_canonical_unitigs(b._h, k, min_count, min_edge, None, None, None, None, None, 0, 0, None, None) == _lib.ERR_NOT_LOADED
            assert lib.msbwt_rle_enumerate_canonical_unitigs_device(b._h, k, min_count, min_edge, None, None, None, None, None, 0, 0, C.byref(u), C.byref(s),
                                                                    None) == _lib.ERR_NOT_LOADED
    assert lib.msbwt_rle_last_error(b._h) == b"no BWT loaded"
    assert (u.value, s.value) == (77, 78) and all((a == 7).all() for a in bufs)  # refused before anything was written
    assert lib.msbwt_rle_canonical_unitig_info(b._h, None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_canonical_unitig_info(b._h, _ptr(info)) == 0 and not info.any()  # nothing called yet
    with pytest.raises(msbwt.MsbwtError) as err:
        b.enumerate_canonical_unitigs(21)
    assert err.value.code == _lib.ERR_NOT_LOADED and "no BWT loaded" in str(err.value)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.enumerate_canonical_unitigs_device(21, None, None, None, None, None, 0, 0, min_count=2, min_edge=3)
    assert err.value.code == _lib.ERR_NOT_LOADED
    assert b.canonical_unitig_info() == dict.fromkeys(INFO, 0)
    assert b.unitig_info()["nodes"] == 0 and b.spectrum_info()["k"] == 0 and b.spectrum_scratch_bytes() == 0


def formula(walk, n, u, s):
    """the header's sum, term by term; walk = msbwt_canonical_plan(total_rows, free_hbm_bytes, 0)"""
    slots = 2 * n
    tiles = (slots + 4095) // 4096
    nodes = (walk + 256 + 128 * n + 32 * min(slots, 2 ** 20) + 2048 * tiles + 8 * ((tiles + 3) // 4 + 8) + 16 * ((slots + 2047) // 2048) + 512 +
             8 * ((slots + 3) // 4))
    if u == 0 and s == 0:
        return nodes  # the counting call
    return nodes + 8 * u + 256 + 8 * u + 8 * ((s + 7) // 8) + 16 * ((u + 7) // 8)


def test_plan_is_the_canonical_walks_plus_the_stated_terms():
    plan, walk = msbwt.canonical_unitigs_plan, msbwt.canonical_plan
    rows = (0, 1, 1023, 1024, 1025, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 40 - 1)
    records = (0, 1, 2, 3, 4, 5, 7, 8, 10, 1023, 1024, 1025, 2047, 2048, 2049, 2 ** 19 - 1, 2 ** 19, 2 ** 19 + 1, 10 ** 6, 10 ** 6 + 1, 10 ** 9, 2 ** 40 - 1)
    for free in (0, 10 ** 9, FREE):
        for t in rows:
            for n in records:
                w = walk(t, free, 0)
                assert plan(t, free, n) == plan(t, free, n, 0, 0) == formula(w, n, 0, 0), (t, free, n)
                for k in (1, 2, 21, 31):
                    for u in sorted({1, n // 30 + 1, n // 2 + 1, max(n, 1)}):  # 1 <= U <= n; S = n + U (k - 1)
                        s = n + u * (k - 1)
                        assert plan(t, free, n, u, s) == formula(w, n, u, s), (t, free, n, u, s)
        sizes = [plan(t, free, 0) for t in rows]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], free
        for t in (10 ** 6, C4):
            sizes = [plan(t, free, n, n // 20 + 1, n + 30 * (n // 20 + 1)) for n in records]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(set(records)), (free, t)
    # C4 at k = 31 from both strands: some 2.9e8 classes -- 128 bytes a class are the large part, the bytes and the tiles 5 more
    n, u = 290 * 10 ** 6, 10 ** 7
    per_class = (plan(C4, FREE, n) - plan(C4, FREE, 0)) / n
    assert 128 + 4 + 1 < per_class < 128 + 4 + 1.2
    assert plan(C4, FREE, n, u, n + 30 * u) - plan(C4, FREE, n) == 256 + 18 * u + n + 30 * u
    # the unitig call over the same 2 n nodes would take 57 bytes a node
    assert plan(C4, FREE, n) - plan(C4, FREE, 0) < 1.2 * (msbwt.unitigs_plan(C4, FREE, 2 * n) - msbwt.unitigs_plan(C4, FREE, 0))


def test_plan_refuses_what_no_index_can_be():
    for t, n, u in ((2 ** 40, 0, 0), (2 ** 40 + 1, 5, 1), (2 ** 64 - 1, 0, 0), (1000, 2 ** 40, 1), (C4, 2 ** 64 - 1, 1), (C4, 1000, 2 ** 40)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.canonical_unitigs_plan(t, FREE, n, u, n)
        assert err.value.code == _lib.ERR_TOO_LARGE, (t, n, u)
    assert _lib.lib().msbwt_canonical_unitigs_plan(1000, FREE, 10, 2, 18, None) == 0  # the output is optional
    assert _lib.lib().msbwt_canonical_unitigs_plan(2 ** 40, FREE, 10, 2, 18, None) == _lib.ERR_TOO_LARGE


def _link_flags():
    return ["-L", LIBDIR, "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "canonical_unitigs")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "canonical_unitigs.c"), "-o", exe] + _link_flags())
    for args in ([], ["-h"], ["x.npy"], ["x.npy", "0"], ["x.npy", "32"], ["x.npy", "21", "0"], ["x.npy", "21", "2", "more"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and r.stdout == ""


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "msbwt_hip.hpp"\n'
                   "int main() {\n"
                   "    const std::uint64_t walk = msbwt::RleBWT::canonical_plan(1000000, 0, 0);\n"
                   "    const std::uint64_t nodes = walk + 256 + 1280 + 640 + 2048 + 72 + 16 + 512 + 40;\n"
                   "    if (msbwt::RleBWT::canonical_unitigs_plan(1000000, 0, 10) != nodes) return 1;\n"
                   "    if (msbwt::RleBWT::canonical_unitigs_plan(1000000, 0, 10, 2, 18) != nodes + 16 + 256 + 16 + 24 + 16) return 1;\n"
                   "    try { msbwt::RleBWT::canonical_unitigs_plan(std::uint64_t(1) << 40, 0); return 1; } catch (const msbwt::Panic &p) { if (p.code != MSBWT_ERR_TOO_LARGE) return 1; }\n"
                   "    msbwt::RleBWT::Unitigs (msbwt::RleBWT::*dump)(std::size_t, std::uint64_t, std::uint64_t) const = &msbwt::RleBWT::enumerate_canonical_unitigs;\n"
                   "    std::uint64_t (msbwt::RleBWT::*device)(std::size_t, std::uint64_t, std::uint64_t, void *, void *, void *, void *, void *, std::uint64_t, std::uint64_t,\n"
                   "                                            std::uint64_t *, void *) const = &msbwt::RleBWT::enumerate_canonical_unitigs_device;\n"
                   "    msbwt::RleBWT::CanonicalUnitigInfo (msbwt::RleBWT::*info)() const = &msbwt::RleBWT::canonical_unitig_info;\n"
                   "    msbwt::RleBWT::CanonicalUnitigInfo i;\n"
                   "    return dump && device && info && i.classes == 0 && i.edge_classes == 0 && i.palindromes == 0 && i.cut_links == 0 && i.rounds == 0 ? 0 : 1;\n"
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
        for method in ("pub fn enumerate_canonical_unitigs(&self", "pub unsafe fn enumerate_canonical_unitigs_device(&self", "pub fn canonical_unitig_info(&self",
                       "pub fn canonical_unitigs_plan("):
            assert method in text
