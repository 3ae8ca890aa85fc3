"""Where the arrays of the by-source block lie (unitig_source_layout of csrc/graph_layouts.hpp), on the host, in the manner of
tests/test_link_layouts.py: tests/cpp/colour_layouts.cpp, a stand-alone program built with AddressSanitizer and UBSan, checks the
layout at each side of every rounding -- alignment, no overlap, the end inside the block's bytes -- and prints the bytes of each; here
the two plans of the public header are held to them: a plan is the graph call's plan plus the layout with its matrix staged."""
import importlib
import os
import subprocess

from conftest import ROOT

msbwt = importlib.import_module("rust-msbwt_amd")


def test_every_array_has_its_own_aligned_place_and_the_plans_take_the_layout(tmp_path):
    exe = str(tmp_path / "colour_layouts")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # (the kernel headers include hip_runtime_api.h for hipError_t; nothing is linked)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "rust-msbwt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "colour_layouts.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    layouts = [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("layout ")]
    assert len(layouts) == 12 * 10 * 5 * 2 and ", 0 failures" in r.stdout
    pad = lambda x: (x + 255) // 256 * 256
    rows, free, seen = 10 ** 9, 250 * 10 ** 9, 0
    for R, U, S, staged, size in layouts:
        assert size == pad(8 * R) + (pad(8 * U * S) if staged else 0), (R, U, S, staged)
        # a plan: R is what the call of `n` nodes (classes) keeps
        if not staged or U == 0 or U >= 2 ** 40 - 1 or R == 0 or R >= 2 ** 40 - 1:
            continue
        for canonical in (False, True):
            n = R if not canonical else (R // 4 if R < 2 ** 21 else 2 ** 30)
            if canonical and (R % 4 or R > 2 ** 21) or U > n:
                continue
            symbols, links = n + 20 * U, 3 * U
            graph = msbwt.unitig_graph_plan(rows, free, n, U, symbols, links, canonical=canonical)
            assert msbwt.unitig_graph_by_source_plan(rows, free, n, U, symbols, links, n_sources=S, canonical=canonical) == graph + size, (R, U, S, canonical)
            assert msbwt.unitig_graph_by_source_plan(rows, free, n, n_sources=S, canonical=canonical) == msbwt.unitig_graph_plan(rows, free, n, canonical=canonical)
            seen += 1
    assert seen > 100
