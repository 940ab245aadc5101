"""The record buffer's layout (msf_loam_amd/csrc/msfl_record_tiles.h): plane records in lane-transposed tiles of 64 rows, then the
edge records.  The header's index functions, compiled with plain g++ (tests/cpp/record_tiles_check.cpp), against a numpy restatement,
and the properties every kernel relies on: no two records share a byte, the plane tiles end where the edge region starts, everything
lies inside what the host reserves, and the 5-NN list a tile holds before the fit lies inside the tile of its own slot."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CORNER = 70


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("record_tiles") / "record_tiles_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "msf_loam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "record_tiles_check.cpp"), "-o", out])
    return out


def model(n_corner, n_surf):
    """numpy restatement: plane slot g -> tile g // 64, lane g % 64; a tile is 256 doubles = {N.x, N.y} x 64 then {N.z, N.C} x 64."""
    g = np.arange(n_surf, dtype=np.int64)
    tile, lane = g // 64, g % 64
    xy = 256 * tile + 2 * lane
    region = 256 * ((n_surf + 63) // 64)
    return {"xy": xy, "zc": xy + 128, "elem": np.stack([xy, xy + 1, xy + 128, xy + 129], 1), "nn4": 2048 * tile + 16 * lane,
            "nn1": 2048 * tile + 1024 + 4 * lane, "region": region, "edge": region + 6 * np.arange(n_corner, dtype=np.int64),
            "buffer": region + 6 * n_corner, "reserved": max(6 * max(n_corner + n_surf, 1), region + 6 * n_corner)}


@pytest.mark.parametrize("n_surf", [0, 1, 63, 64, 65, 4097])
def test_tile_addresses(exe, n_surf):
    lines = subprocess.check_output([exe, str(N_CORNER), str(n_surf)], text=True).split("\n")
    head = [int(x) for x in lines[0].split()[1:]]
    slots = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("slot")], np.int64).reshape(-1, 9)
    edges = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("edge")], np.int64).reshape(-1, 2)
    m = model(N_CORNER, n_surf)
    # the numpy restatement gives the same addresses
    assert head == [m["region"], m["buffer"], m["reserved"]]
    assert len(slots) == n_surf and np.array_equal(slots[:, 0], np.arange(n_surf))
    assert np.array_equal(slots[:, 1], m["xy"]) and np.array_equal(slots[:, 2], m["zc"]) and np.array_equal(slots[:, 3:7], m["elem"])
    assert np.array_equal(slots[:, 7], m["nn4"]) and np.array_equal(slots[:, 8], m["nn1"])
    assert np.array_equal(edges[:, 0], np.arange(N_CORNER)) and np.array_equal(edges[:, 1], m["edge"])
    # every record's bytes: disjoint from each other, planes disjoint from the edge region, all inside the reserved size
    owner = np.full(8 * m["reserved"], -1, np.int64)
    def claim(byte0, n_bytes, who):
        for b0, w in zip(np.atleast_1d(byte0), np.atleast_1d(who)):
            assert 0 <= b0 and b0 + n_bytes <= len(owner), (b0, n_bytes)
            assert np.all(owner[b0:b0 + n_bytes] == -1), ("overlap", w)
            owner[b0:b0 + n_bytes] = w
    claim(8 * slots[:, 1], 16, slots[:, 0]); claim(8 * slots[:, 2], 16, slots[:, 0])
    assert np.all(8 * slots[:, 2] + 16 <= 8 * m["region"]) and m["region"] % 256 == 0          # planes end before the edge region
    claim(8 * edges[:, 1], 48, n_surf + edges[:, 0])
    assert np.all(edges[:, 1] >= m["region"])
    # the four elements are the two double2 halves; 16-byte alignment of both halves
    assert np.array_equal(slots[:, 3], slots[:, 1]) and np.array_equal(slots[:, 5], slots[:, 2]) and np.all(slots[:, 1:3] % 2 == 0)
    # neighbour lists: inside the slot's own tile, disjoint from each other, whole 16- and 4-byte aligned pieces
    tile0 = 2048 * (slots[:, 0] // 64)
    assert np.all(slots[:, 7] >= tile0) and np.all(slots[:, 7] + 16 <= tile0 + 1024)
    assert np.all(slots[:, 8] >= tile0 + 1024) and np.all(slots[:, 8] + 4 <= tile0 + 1280)
    assert np.all(slots[:, 7] % 16 == 0) and np.all(slots[:, 8] % 4 == 0)
    assert len(set(slots[:, 7])) == n_surf and len(set(slots[:, 8])) == n_surf
    assert np.all(slots[:, 8] + 4 <= 8 * m["region"])
    # a wavefront's 64 consecutive rows of one tile are two contiguous kilobytes
    if n_surf >= 64:
        assert np.array_equal(np.diff(slots[:64, 1]), np.full(63, 2)) and slots[63, 1] + 2 == slots[0, 2]
