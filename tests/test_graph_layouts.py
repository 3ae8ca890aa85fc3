"""Where the arrays of the graph's and the unitigs' HBM blocks lie (csrc/graph_layouts.hpp), on the host: tests/cpp/graph_layouts.cpp,
a stand-alone program built with AddressSanitizer and UBSan, checks every layout at each side of every rounding -- alignment, no
overlap, the end at the block's bytes, the zeroed span, the overlays inside what they lie over.  The totals are pinned elsewhere: the
*_abi tests hold every plan against the public header's sum."""
import os
import subprocess

from conftest import ROOT


def test_every_array_has_its_own_aligned_place(tmp_path):
    exe = str(tmp_path / "graph_layouts")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # (the kernel headers include hip_runtime_api.h for hipError_t; nothing is linked)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "rust-msbwt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "graph_layouts.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    # 14 sizes of three node blocks (the canonical one under both outcomes of the sort) and 4 x 4 x 16 output blocks
    assert "graph layouts: 4022 checks, 0 failures" in r.stdout
