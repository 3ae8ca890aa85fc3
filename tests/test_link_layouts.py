"""Where the arrays of the link table's HBM block lie (unitig_link_layout of csrc/graph_layouts.hpp), on the host, in the manner of
tests/test_graph_layouts.py: tests/cpp/link_layouts.cpp, a stand-alone program built with AddressSanitizer and UBSan, checks the layout
at each side of every rounding -- alignment, no overlap, the end at the block's bytes -- and prints the bytes of each; here the two
plans of the public header are held to them: a plan is the unitig call's plan plus the layout with its targets staged."""
import importlib
import os
import subprocess

from conftest import ROOT

msbwt = importlib.import_module("rust-msbwt_amd")


def test_every_array_has_its_own_aligned_place_and_the_plans_take_the_layout(tmp_path):
    exe = str(tmp_path / "link_layouts")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # (the kernel headers include hip_runtime_api.h for hipError_t; nothing is linked)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "rust-msbwt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "link_layouts.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    layouts = [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("layout ")]
    # 10 sizes x 5 numbers of links x staged or not, 9 checks with the targets and 7 without
    assert len(layouts) == 100 and "link layouts: 800 checks, 0 failures" in r.stdout
    rows, free, seen = 10 ** 9, 250 * 10 ** 9, 0
    for U, L, staged, size in layouts:
        assert size == 16 * U + 256 + 16 * ((2 * U + 1 + 2047) // 2048) + (8 * L if staged else 0), (U, L, staged)
        if not staged or U == 0 or U >= 2 ** 40 - 1:
            continue
        for canonical, plan in ((False, msbwt.unitigs_plan), (True, msbwt.canonical_unitigs_plan)):
            n, S = 3 * U, 3 * U + 20 * U
            assert msbwt.unitig_graph_plan(rows, free, n, U, S, L, canonical=canonical) == plan(rows, free, n, U, S) + size, (U, L, canonical)
            assert msbwt.unitig_graph_plan(rows, free, n, canonical=canonical) == plan(rows, free, n), (U, canonical)  # the counting call
            seen += 1
    assert seen == 2 * 5 * 8
