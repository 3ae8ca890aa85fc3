"""The merge entry points (include/msbwt_hip.h: msbwt_rle_merge and its companions) without a GPU: the symbols and their
signatures, a plain-C host, the argument guards, the memory plan, the shim's two copies."""
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
NEW = ("msbwt_rle_merge", "msbwt_rle_load_merged", "msbwt_merge_plan", "msbwt_merge_tile", "msbwt_rle_merge_info")


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p,
                "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "double *": C.POINTER(C.c_double), "size_t": C.c_size_t, "uint64_t": C.c_uint64,
                "int": C.c_int}
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
    assert msbwt.merge_tile() >= 64 and msbwt.merge_tile() % 64 == 0
    assert len(_lib.MERGE_STAGES) == 6


def _compile(src, out, std):
    subprocess.check_call(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", LIBDIR,
                           "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def test_plain_c_host_compiles_and_its_guards_answer_without_a_device(tmp_path):
    exe = str(tmp_path / "merge_abi")
    _compile(os.path.join(ROOT, "tests", "cpp", "merge_abi.c"), exe, "c11")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "merge_bwts")
    _compile(os.path.join(ROOT, "examples", "merge_bwts.c"), exe, "c11")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_python_guards_answer_without_a_device():
    b = msbwt.RleBWT()
    ok = np.array([1 | 3 << 3, 0 | 1 << 3], dtype=np.uint8)
    for bad, code in (([6 | 1 << 3], _lib.ERR_INVALID_SYMBOL), ([7], _lib.ERR_INVALID_SYMBOL), ([0xF9] * 9, _lib.ERR_TOO_LARGE)):
        for pair in ((bad, ok), (ok, bad)):
            for call in (b.merge, b.load_merged, lambda x, y: b.merge(x, y, return_interleave=True)):
                with pytest.raises(msbwt.MsbwtError) as err:
                    call(*pair)
                assert err.value.code == code
    half = [1] * 7 + [1 | 16 << 3]  # 2^39 'A'
    assert msbwt.rle_bwt.rle_total(half) == 2 ** 39
    with pytest.raises(msbwt.MsbwtError) as err:
        b.merge(half, half)
    assert err.value.code == _lib.ERR_TOO_LARGE
    merged, bits = b.merge([], [], return_interleave=True)
    assert merged.size == 0 and bits.size == 0
    assert b.merge_info()["iterations"] == 0
    assert b.get_total_size() == 0


def test_rle_helpers():
    rle = np.array([1 | 24 << 3, 1 | 18 << 3, 0, 1 | 1 << 3, 2 | 31 << 3, 2 | 0 << 3, 2 | 1 << 3], dtype=np.uint8)
    assert msbwt.rle_bwt.rle_total(rle) == 600 + 1 + 31 + 1024
    codes = msbwt.rle_bwt.rle_decode(rle)
    assert codes.dtype == np.uint8 and codes.tolist() == [1] * 601 + [2] * 1055
    assert msbwt.rle_bwt.rle_total([]) == 0 and msbwt.rle_bwt.rle_decode([]).size == 0


C4_HALF, HUMAN_HALF = 1_950_000_000, 45_000_000_000


def test_plan_is_monotone_symmetric_and_within_its_bound():
    for t0, t1 in ((1, 1), (C4_HALF, C4_HALF), (HUMAN_HALF, HUMAN_HALF), (0, 5), (12345, 1)):
        size = msbwt.merge_plan(t0, t1)
        assert size == msbwt.merge_plan(t1, t0)
        assert 2 * (t0 + t1) <= size <= 2.5 * (t0 + t1) + (64 << 20)
    steps = (0, 1, 10 ** 6, 10 ** 8, C4_HALF, HUMAN_HALF, 2 ** 39)
    for other in (0, 1, 10 ** 8, 2 ** 39 - 1):
        sizes = [msbwt.merge_plan(t, other) for t in steps if t + other < 2 ** 40]
        assert sizes == sorted(sizes) and len(set(sizes[1:])) == len(sizes[1:])
        assert sizes == [msbwt.merge_plan(other, t) for t in steps if t + other < 2 ** 40]
    for t0, t1 in ((2 ** 40, 0), (0, 2 ** 40), (2 ** 39, 2 ** 39), (2 ** 40 - 1, 1)):
        with pytest.raises(msbwt.MsbwtError) as err:
            msbwt.merge_plan(t0, t1)
        assert err.value.code == _lib.ERR_TOO_LARGE
    assert msbwt.merge_plan(2 ** 40 - 2, 1) > 2 * 2 ** 40


# ---- the Rust shim ----

def test_both_shim_copies_declare_the_merge_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in NEW[:2]:
        assert name in a, name
    for text in (shim.SOURCES["shim/msbwt2-hip/src/lib.rs"](), shim.SOURCES["INTEGRATION.md"]()):
        assert "pub fn merge(&mut self" in text
