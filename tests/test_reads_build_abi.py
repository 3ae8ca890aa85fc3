"""The construction entry points (include/msbwt_hip.h: msbwt_rle_build_from_reads and its companions) without a GPU: the symbols
and their signatures, a plain-C host, the argument guards, the memory plan, the FASTA/FASTQ reader, the shim's two copies."""
import ctypes as C
import gzip
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
LIBDIR = os.path.join(ROOT, "rust-msbwt_amd")
NEW = ("msbwt_rle_build_from_reads", "msbwt_rle_load_reads", "msbwt_rle_set_build_piece", "msbwt_build_reads_plan",
       "msbwt_build_reads_sort_tile", "msbwt_rle_build_stage_ms")


def test_symbols_load_with_the_declared_signatures():
    import test_shim_matches_header as shim
    decls = shim.c_declarations()
    ctype_of = {"msbwt_rle *": C.c_void_p, "const msbwt_rle *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p,
                "const uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)), "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64)),
                "double *": C.POINTER(C.c_double), "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int": C.c_int}
    for name in NEW:
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SIGNATURES[name]
        cret, cparams = decls[name]
        assert ctype_of[shim.norm_c(cret)] == res
        assert len(cparams) == len(args), name
        for ct, a in zip(cparams, args):
            want = ctype_of[shim.norm_c(ct)]
            assert a in want if isinstance(want, tuple) else a == want, (name, ct)
    assert _lib.lib().msbwt_build_reads_sort_tile() >= 64


def _compile(src, out, std):
    subprocess.check_call(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", LIBDIR,
                           "-lmsbwt_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def test_plain_c_host_compiles_and_its_guards_answer_without_a_device(tmp_path):
    exe = str(tmp_path / "reads_build_abi")
    _compile(os.path.join(ROOT, "tests", "cpp", "reads_build_abi.c"), exe, "c11")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "build_from_reads")
    _compile(os.path.join(ROOT, "examples", "build_from_reads.c"), exe, "c11")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_python_guards_answer_without_a_device():
    b = msbwt.RleBWT()
    for reads, ascii in (([bytes([1, 0])], False), ([bytes([7])], False), (["A$"], True)):
        for call in (b.build_from_reads, b.load_reads):
            with pytest.raises(msbwt.MsbwtError) as err:
                call(reads, ascii=ascii)
            assert err.value.code == _lib.ERR_INVALID_SYMBOL
    flat = np.array([1, 2, 3], dtype=np.uint8)
    with pytest.raises(msbwt.MsbwtError) as err:
        b.build_from_reads((flat, np.array([0, 3, 2], dtype=np.uint64)))
    assert err.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(TypeError):
        b.build_from_reads(["ACGT"])  # text needs ascii=True
    assert b.build_from_reads([]).size == 0
    with pytest.raises(NotImplementedError):
        msbwt.create_from_fastx(os.path.join(GOLDEN_DIR, "two_string.fa"), sorted=False)


def test_pack_reads():
    flat, offsets = msbwt.rle_bwt.pack_reads(["AC", "", "GGT"], ascii=True)
    assert flat.tobytes() == b"ACGGT" and offsets.tolist() == [0, 2, 2, 5]
    flat, offsets = msbwt.rle_bwt.pack_reads([np.array([1, 2]), bytes([5])])
    assert flat.tolist() == [1, 2, 5] and offsets.tolist() == [0, 2, 3]
    same = msbwt.rle_bwt.pack_reads((flat, offsets))
    assert same[0].tolist() == [1, 2, 5] and same[1].tolist() == [0, 2, 3]


C4_TOTAL, HUMAN_TOTAL = 1_946_213_783, 90_000_000_000


def test_plan_is_monotone_and_large_enough():
    hbm = 288 << 30
    for total in (C4_TOTAL, HUMAN_TOTAL, 1, 12345):
        piece, size = msbwt.build_reads_plan(total, hbm)
        assert piece >= 1 and size >= 2 * total
    # more free HBM: never a smaller piece; more symbols: never a larger one
    pieces = [msbwt.build_reads_plan(C4_TOTAL, free)[0] for free in (0, 1 << 30, 8 << 30, 64 << 30, 288 << 30)]
    assert pieces == sorted(pieces) and pieces[0] == 1 and pieces[-1] > pieces[0]
    pieces = [msbwt.build_reads_plan(total, hbm)[0] for total in (10 ** 6, 10 ** 8, C4_TOTAL, HUMAN_TOTAL)]
    assert pieces == sorted(pieces, reverse=True)
    # the bytes grow with the symbols and with the piece
    sizes = [msbwt.build_reads_plan(total, hbm, 1 << 20)[1] for total in (10 ** 6, 10 ** 8, C4_TOTAL, HUMAN_TOTAL)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    sizes = [msbwt.build_reads_plan(C4_TOTAL, hbm, piece)[1] for piece in (1, 1000, 1 << 20, 1 << 28, 1 << 36)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[3]
    # the automatic piece's own need fits what was called free
    for free in (8 << 30, 64 << 30, 288 << 30):
        piece, size = msbwt.build_reads_plan(C4_TOTAL, free)
        assert size <= free or piece == 1
    with pytest.raises(msbwt.MsbwtError):
        msbwt.build_reads_plan(1 << 40, hbm)


# ---- the FASTA / FASTQ reader ----

dyn = msbwt.dynamic_bwt
FASTA = b">r1 first\nACGT\nacgt\n\n>r2\nNNRY-.\n>empty\n>r4\nTTTT\r\nU u\n"
FASTQ = b"@q1\nACGTN\n+\nIIIII\n@q2 x\nacg\n+q2\n@@@\n"


def _codes(reads):
    return [r.tolist() for r in reads]


def test_reader_on_the_golden_fasta():
    assert _codes(dyn.reads_from_fastx(os.path.join(GOLDEN_DIR, "two_string.fa"))) == [[1, 2, 3, 5], [5, 3, 2, 1]]


def test_reader_on_multi_line_fasta_lower_case_and_other_bytes(tmp_path):
    p = tmp_path / "a.fa"
    p.write_bytes(FASTA)
    records = list(dyn.read_fastx(str(p)))
    assert [name for name, _ in records] == [b"r1 first", b"r2", b"empty", b"r4"]
    assert _codes(dyn.reads_from_fastx(str(p))) == [[1, 2, 3, 5, 1, 2, 3, 5], [4] * 6, [], [5, 5, 5, 5, 5, 5]]
    # the same bytes through the library's own ASCII mapping, blanks removed and U read as T as needletail's normalize does
    assert dyn.sequence_codes(b"acgtNx$").tolist() == msbwt.string_util.convert_stoi(b"acgtNxN").tolist()


def test_reader_on_fastq_and_gzip(tmp_path):
    q = tmp_path / "a.fq"
    q.write_bytes(FASTQ)
    assert _codes(dyn.reads_from_fastx(str(q))) == [[1, 2, 3, 5, 4], [1, 2, 3]]
    for name, text in (("a.fa.gz", FASTA), ("a.fq.gz", FASTQ)):
        with gzip.open(str(tmp_path / name), "wb") as f:
            f.write(text)
    assert _codes(dyn.reads_from_fastx(str(tmp_path / "a.fq.gz"))) == [[1, 2, 3, 5, 4], [1, 2, 3]]
    both = dyn.reads_from_fastx([str(tmp_path / "a.fa.gz"), str(q)])
    assert len(both) == 6 and both[0].tolist() == [1, 2, 3, 5, 1, 2, 3, 5] and both[5].tolist() == [1, 2, 3]
    bad = tmp_path / "bad.txt"
    bad.write_bytes(b"ACGT\n")
    with pytest.raises(ValueError):
        dyn.reads_from_fastx(str(bad))


# ---- the Rust shim ----

def test_both_shim_copies_declare_the_builders_alike():
    import test_shim_matches_header as shim
    a = shim.rust_declarations(shim.SOURCES["shim/msbwt2-hip/src/lib.rs"]())
    b = shim.rust_declarations(shim.SOURCES["INTEGRATION.md"]())
    assert a == b
    for name in NEW[:4]:
        assert name in a, name
