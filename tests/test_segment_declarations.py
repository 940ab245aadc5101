"""The new declarations of include/msfl_c_api.h (msfl_segment_scans, msfl_segment_scan, msfl_segment_tables,
msfl_segment_default_config and their two records) as C99 and through the C++ mirror (ScanRegistration::Segment,
include/msfl/scan_matcher.hpp): compiled on the CPU, run on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = "-I" + os.path.join(ROOT, "include")


def test_the_header_compiles_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", INC, "-c", os.path.join(ROOT, "tests", "cpp", "segment_check_c.c"),
                           "-o", str(tmp_path / "segment_check_c.o")])


def test_the_cpp_mirror_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", INC, "-c", os.path.join(ROOT, "tests", "cpp", "segment_check.cpp"),
                           "-o", str(tmp_path / "segment_check.o")])


@pytest.mark.gpu
def test_cpp_mirror_segments(gpu, tmp_path):
    exe = str(tmp_path / "segment_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", INC, os.path.join(ROOT, "tests", "cpp", "segment_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("segment_check ok: 7200 ground, 48 segment, 1 outlier")
