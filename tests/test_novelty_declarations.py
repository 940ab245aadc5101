"""The new declarations of include/msfl_c_api.h (msfl_grid_render, msfl_novelty_default_config, msfl_scan_novelty,
msfl_grids_scan_novelty and their records) as C99 and through the C++ mirror (HybridGrid::Render, ScanNovelty,
include/msfl/scan_matcher.hpp): compiled on the CPU, run on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = "-I" + os.path.join(ROOT, "include")


def test_the_header_compiles_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", INC, "-c", os.path.join(ROOT, "tests", "cpp", "novelty_check_c.c"),
                           "-o", str(tmp_path / "novelty_check_c.o")])


def test_the_cpp_mirror_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", INC, "-c", os.path.join(ROOT, "tests", "cpp", "novelty_check.cpp"),
                           "-o", str(tmp_path / "novelty_check.o")])


@pytest.mark.gpu
def test_cpp_mirror_renders_and_labels(gpu, tmp_path):
    exe = str(tmp_path / "novelty_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", INC, os.path.join(ROOT, "tests", "cpp", "novelty_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("novelty_check ok: 0 none, 12 unseen, 116 covered, 8 in front")
