"""Host-side safety of the plane conv (csrc/conv2d.hip): its tile, mask and workspace index
arithmetic lives in csrc/conv2d_geom.h; tools/conv2d_geom_check.cpp restates the kernels' loops
on the host and walks them over 1912 geometries with bounds-checked accesses (std::vector::at).
Built here as a stand-alone program under the undefined-behaviour sanitizer (without it where
the compiler has none) and run on the CPU; the program also builds with -fsanitize=address."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_walk(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "conv2d_geom_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(REPO, "dl-swin-gan_amd", "csrc"),
            os.path.join(REPO, "tools", "conv2d_geom_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert run.stdout.startswith("ok: 1912 geometries")
