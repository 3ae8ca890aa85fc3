"""The k-mer range and extension entry points (include/msbwt_hip.h) from a plain C host: examples/kmer_extensions.c calls all
four and links against libmsbwt_hip.so.  Without arguments it only prints its usage (no GPU touched); on a GPU box it runs."""
import os
import subprocess

import pytest

from conftest import GOLDEN_DIR, ROOT

LIBDIR = os.path.join(ROOT, "rust-msbwt_amd")


def _build_example(out):
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "kmer_extensions.c"), "-o", out, "-L", LIBDIR, "-lmsbwt_hip",
                           "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])


def test_extensions_example_compiles_and_links(tmp_path):
    exe = str(tmp_path / "kmer_extensions")
    _build_example(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_python_binding_declares_the_four_entry_points():
    import importlib
    lib = importlib.import_module("rust-msbwt_amd._lib")
    for name in ("msbwt_rle_kmer_ranges", "msbwt_rle_kmer_ranges_device", "msbwt_rle_count_kmer_extensions",
                 "msbwt_rle_count_kmer_extensions_device"):
        assert name in lib.SIGNATURES
        assert hasattr(lib.lib(), name)


@pytest.mark.gpu
def test_extensions_example_on_two_string(tmp_path):
    # two_string.npy holds the strings of naive_bwt(["ACGT", "TGCA"]): ACG occurs once, preceded by '$'; CGT once, preceded by A
    exe = str(tmp_path / "kmer_extensions")
    _build_example(exe)
    r = subprocess.run([exe, os.path.join(GOLDEN_DIR, "two_string.npy"), "ACG", "CGT", "GGG"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {line.split("\t")[0]: line.split("\t")[1:] for line in r.stdout.splitlines() if "\t" in line}
    acg, cgt, ggg = ([int(x) for x in rows[q]] for q in ("ACG", "CGT", "GGG"))
    assert acg[1] - acg[0] == 1 and acg[2:] == [1, 0, 0, 0, 0, 0]
    assert cgt[1] - cgt[0] == 1 and cgt[2:] == [0, 1, 0, 0, 0, 0]
    assert ggg == [0, 0, 0, 0, 0, 0, 0, 0]
    assert "device forms agree" in r.stdout
