"""The lookup kernel's bucket scan (csrc/lookup_kernel.hpp) on the host: tests/cpp/lookup_scan_host.cpp, a stand-alone program built
with AddressSanitizer and UBSan, fills buckets of the three complete layouts through their descriptors -- a full bucket, chains of
`probe`, the escape width, the table's last line -- and counts present and absent keys with the functions the kernel runs."""
import os
import subprocess

from conftest import ROOT


def test_the_shared_scan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lookup_scan_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rust-msbwt_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lookup_scan_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lookup scan: all host checks passed" in r.stdout and r.stdout.count("depth ") == 6
