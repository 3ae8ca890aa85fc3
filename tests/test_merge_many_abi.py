"""The one-pass merge entry points (include/msbwt_hip.h: msbwt_rle_merge_many and its companions) without a GPU: the symbols and
their signatures, a plain-C host, the argument guards, the empty merges, the memory plan, the example, the shim's two copies."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
LIBDIR = os.path.join(ROOT, "rust-msbwt_amd")
NEW = ("msbwt_rle_merge_many", "msbwt_rle_load_merged_many", "msbwt_merge_many_plan")


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p, "const uint64_t *": C.c_void_p,
                "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "size_t": C.c_size_t, "int": C.c_int}
    for name in NEW:
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SIGNATURES[name]
        cret, cparams = decls[name]
        assert ctype_of[shim.norm_c(cret)] == res
        assert len(cparams) == len(args), name
        for ct, a in zip(cparams, args):
            assert shim.norm_c(ct) in shim.C_TO_RUST, (name, ct)
            want = ctype_of[shim.norm_c(ct)]
            assert a in want if isinstance(want, tuple) else a == want, (name, ct)
    assert [shim.norm_c(t) for t in decls["msbwt_rle_merge_many"][1]] == ["msbwt_rle *", "const uint8_t *", "const uint64_t *", "size_t", "uint8_t *", "size_t",
                                                                         "uint64_t *", "uint8_t *"]
    assert msbwt.MERGE_MAX_INPUTS == _lib.MERGE_MAX_INPUTS == 32
    assert "#define MSBWT_MERGE_MAX_INPUTS 32" in open(os.path.join(ROOT, "include", "msbwt_hip.h")).read()


def _compile(src, out, std):
    subprocess.check_call(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", LIBDIR,
                           "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def test_plain_c_host_compiles_and_its_guards_answer_without_a_device(tmp_path):
    exe = str(tmp_path / "merge_many_abi")
    _compile(os.path.join(ROOT, "tests", "cpp", "merge_many_abi.c"), exe, "c11")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "merge_many_bwts")
    _compile(os.path.join(ROOT, "examples", "merge_many_bwts.c"), exe, "c11")
    for args in ([], ["a.npy", "b.npy"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_empty_merges_touch_no_device():
    b = msbwt.RleBWT()
    for rles in ([], [[]] * 32, [np.empty(0, dtype=np.uint8)] * 3, [[0, 1 | 0 << 3]]):  # (the last: zero digits only)
        merged, sources = b.merge_many(rles, return_sources=True)
        assert merged.dtype == np.uint8 and merged.size == 0 and sources.size == 0
        assert b.merge_many(rles).size == 0
        assert b.merge_info()["iterations"] == 0
    assert b.get_total_size() == 0
    assert msbwt.bwt_util.multi_bwt_merge(["", "", ""]) == ""


def test_python_guards_answer_without_a_device():
    b = msbwt.RleBWT()
    ok = np.array([1 | 3 << 3, 0 | 1 << 3], dtype=np.uint8)
    for bad, code in (([6 | 1 << 3], _lib.ERR_INVALID_SYMBOL), ([7], _lib.ERR_INVALID_SYMBOL), ([0xF9] * 9, _lib.ERR_TOO_LARGE)):
        for rles in ((bad, ok, ok), (ok, ok, bad), (ok, [], bad, ok)):
            for call in (b.merge_many, b.load_merged_many, lambda r: b.merge_many(r, return_sources=True)):
                with pytest.raises(msbwt.MsbwtError) as err:
                    call(rles)
                assert err.value.code == code
    with pytest.raises(msbwt.MsbwtError) as err:
        b.merge_many([ok, ok, [6 | 1 << 3]])
    assert "input 2" in str(err.value)
    half = [1] * 7 + [1 | 16 << 3]  # 2^39 'A'
    for call in (b.merge_many, b.load_merged_many):
        with pytest.raises(msbwt.MsbwtError) as err:
            call([half, [], half])
        assert err.value.code == _lib.ERR_TOO_LARGE
        with pytest.raises(msbwt.MsbwtError) as err:
            call([ok] * 33)
        assert err.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        msbwt.bwt_util.merge_numpy_files([], "nowhere.npy", method="one_pass")
    with pytest.raises(ValueError):
        msbwt.bwt_util.merge_numpy_files([], "nowhere.npy", method="fastest")


C4, HUMAN = 3_900_000_000, 90_000_000_000


def test_plan_is_symmetric_monotone_and_within_its_bounds():
    plan = msbwt.merge_many_plan
    for totals in ((1, 1, 1), (C4 // 4,) * 4, (C4 // 2, C4 // 4, C4 // 8, C4 // 8), (HUMAN // 8,) * 8, (HUMAN // 32,) * 32, (0, 5, 0), (12345, 1, 7, 0, 0)):
        size = plan(totals)
        for other in itertools.islice(itertools.permutations(totals), 24):
            assert plan(other) == size
        assert 2 * sum(totals) <= size <= 3.25 * sum(totals) + (64 << 20)
    steps = (0, 1, 10 ** 6, 10 ** 8, C4, HUMAN, 2 ** 39)
    for others in ((0, 0), (1, 0, 7), (10 ** 8,) * 5, (2 ** 38, 2 ** 38 - 1)):
        for at in range(len(others) + 1):
            sizes = [plan(others[:at] + (t,) + others[at:]) for t in steps if t + sum(others) < 2 ** 40]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert plan([]) == plan([0]) == plan([0] * 32)
    for totals in ((2 ** 40,), (0, 2 ** 40, 0), (2 ** 39, 0, 2 ** 39), (2 ** 40 - 1, 1), (2 ** 38,) * 4, (2 ** 64 - 1, 1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            plan(totals)
        assert err.value.code == _lib.ERR_TOO_LARGE
    assert plan((2 ** 40 - 2, 1)) > 2 * 2 ** 40
    with pytest.raises(msbwt.MsbwtError) as err:
        plan([1] * 33)
    assert err.value.code == _lib.ERR_INVALID_ARG


# ---- the Rust shim ----

def test_both_shim_copies_declare_the_merge_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in NEW[:2]:
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        assert "pub fn merge_many(&mut self" in text
