"""CPU: the keyframe store's declarations as C99 and through the C++ face (include/msfl/keyframes.hpp), its host bookkeeping
(msf_loam_amd/csrc/msfl_keyframes_host.h) as a stand-alone program under the host sanitizers, and the keyframe file format of
msf_loam_amd/mapio.py (numpy only).  One gpu-marked case runs the C++ check end to end."""
import os
import subprocess

import numpy as np
import pytest

from msf_loam_amd import mapio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = "-I" + os.path.join(ROOT, "include")


def test_the_header_compiles_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", INC, "-c", os.path.join(ROOT, "tests", "cpp", "keyframes_check_c.c"),
                           "-o", str(tmp_path / "keyframes_check_c.o")])


def test_the_cpp_face_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", INC, "-c", os.path.join(ROOT, "tests", "cpp", "keyframes_check.cpp"),
                           "-o", str(tmp_path / "keyframes_check.o")])


@pytest.mark.gpu
def test_cpp_face_adds_composes_and_inserts(gpu, tmp_path):
    exe = str(tmp_path / "keyframes_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", INC, os.path.join(ROOT, "tests", "cpp", "keyframes_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("keyframes_check ok: 2 keyframes, 1155 + 2049 points composed")


def test_host_bookkeeping_under_the_host_sanitizers(tmp_path):
    """Member tables for the compose cases of tests/test_gpu_keyframes.py, totals just below and at 2^31, every refusal: a stand-alone
    program built with -fsanitize=address,undefined, run on the CPU."""
    exe = str(tmp_path / "keyframes_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "msf_loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "keyframes_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "keyframes host ok" in out.stdout, out.stderr


def test_python_face_and_exports_name_every_call():
    from msf_loam_amd import capi
    for n in ("default_config", "create", "destroy", "size", "add", "sizes", "get", "compose", "insert"):
        assert "msfl_keyframes_" + n in capi.EXPORTED
    for m in ("add", "add_device", "sizes", "get", "compose", "compose_device", "insert"):
        assert callable(getattr(capi.Keyframes, m))
    assert C_sizeof(capi.KeyframesConfig) == 20


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


# ---- the keyframe file ----------------------------------------------------------------------------------------------------

CFG = dict(max_keyframes=8, max_corner_points=4096, max_surf_points=4096, leaf_corner=0.2, leaf_surf=0.4)


def _store(rng, counts=((5, 9), (0, 3), (7, 0))):
    n_corner = np.array([c for c, _ in counts], np.int32)
    n_surf = np.array([s for _, s in counts], np.int32)
    corner = rng.normal(0, 10, (int(n_corner.sum()), 4)).astype(np.float32)
    surf = rng.normal(0, 10, (int(n_surf.sum()), 4)).astype(np.float32)
    corner[0, 2] = -0.0
    return n_corner, n_surf, corner, surf


def test_keyframe_file_round_trips_byte_for_byte(tmp_path):
    rng = np.random.default_rng(1)
    n_corner, n_surf, corner, surf = _store(rng)
    path = str(tmp_path / "kf.npz")
    mapio.write_keyframes(path, CFG, n_corner, n_surf, corner, surf)
    cfg, nc, ns, c, s = mapio.read_keyframes(path)
    assert cfg == dict(CFG, leaf_corner=float(np.float32(0.2)), leaf_surf=float(np.float32(0.4)))
    assert nc.tobytes() == n_corner.tobytes() and ns.tobytes() == n_surf.tobytes() and nc.dtype == np.int32
    assert c.tobytes() == corner.tobytes() and s.tobytes() == surf.tobytes() and c.dtype == np.float32
    # an empty store is a file too
    mapio.write_keyframes(path, CFG, n_corner[:0], n_surf[:0], corner[:0], surf[:0])
    cfg, nc, ns, c, s = mapio.read_keyframes(path)
    assert len(nc) == len(ns) == 0 and c.shape == (0, 4) and s.shape == (0, 4)


def test_every_validation_rule_refuses_a_crafted_file(tmp_path):
    rng = np.random.default_rng(2)
    n_corner, n_surf, corner, surf = _store(rng)
    path = str(tmp_path / "bad.npz")
    good = dict(keyframes_format=np.int32(mapio.KEYFRAMES_FORMAT), n_corner=n_corner, n_surf=n_surf, corner=corner, surf=surf,
                max_keyframes=np.int32(8), max_corner_points=np.int32(4096), max_surf_points=np.int32(4096), leaf_corner=np.float32(0.2),
                leaf_surf=np.float32(0.4))

    def refused(words, drop=None, **change):
        d = dict(good, **change)
        if drop:
            del d[drop]
        with open(path, "wb") as f:
            np.savez(f, **d)
        with pytest.raises(mapio.MapFileError) as e:
            mapio.read_keyframes(path)
        assert words in str(e.value), str(e.value)

    with open(path, "wb") as f:
        np.savez(f, **good)
    mapio.read_keyframes(path)                                        # the uncrafted file is fine
    for k in good:
        refused("not a keyframe file", drop=k)
    refused("format 2", keyframes_format=np.int32(2))
    refused("1-D int32", n_corner=n_corner.astype(np.int64))
    refused("1-D int32", n_surf=n_surf.reshape(1, -1))
    refused("negative count", n_corner=np.array([13, -1, 0], np.int32))
    refused("keyframes, n_surf", n_surf=np.array([9, 3], np.int32))
    refused("float32 array", corner=corner.astype(np.float64))
    refused("float32 array", surf=surf[:, :3])
    refused("corner counts sum", n_corner=np.array([5, 0, 8], np.int32))
    refused("surf counts sum", surf=surf[:-1])
    for bad in (np.nan, np.inf, -np.inf):
        for coord in range(4):
            c2 = corner.copy(); c2[3, coord] = bad
            refused("corner point is not finite", corner=c2)
            s2 = surf.copy(); s2[-1, coord] = bad
            refused("surf point is not finite", surf=s2)
    refused("max_keyframes < 1", max_keyframes=np.int32(0))
    refused("negative pool", max_surf_points=np.int32(-1))
    refused("leaf_corner", leaf_corner=np.float32(-0.2))
    refused("leaf_surf", leaf_surf=np.float32(np.nan))
    refused("more than its own config", max_keyframes=np.int32(2))
    refused("more than its own config", max_corner_points=np.int32(11))
    refused("more than its own config", max_surf_points=np.int32(11))
    # and the writer applies the same rules
    with pytest.raises(mapio.MapFileError):
        mapio.write_keyframes(path, CFG, n_corner, n_surf, corner[:-1], surf)
    with pytest.raises(mapio.MapFileError):
        mapio.write_keyframes(path, dict(CFG, leaf_surf=-1.0), n_corner, n_surf, corner, surf)


@pytest.mark.gpu
def test_a_store_saved_and_loaded_is_the_same_store(gpu, tmp_path):
    from msf_loam_amd import capi
    rng = np.random.default_rng(3)
    k = capi.Keyframes(gpu, max_keyframes=8, max_corner_points=4096, max_surf_points=4096)       # leaves 0.2 / 0.4
    for n_c, n_s in ((300, 900), (0, 70), (65, 0)):
        k.add(rng.uniform(-2, 2, (n_c, 4)).astype(np.float32), rng.uniform(-2, 2, (n_s, 4)).astype(np.float32))
    path = str(tmp_path / "kf.npz")
    assert mapio.save_keyframes(path, k) == 3
    k2 = mapio.load_keyframes(path, gpu)
    assert k2.size() == 3 and k2.file_config["leaf_surf"] == float(np.float32(0.4)) and k2.config.leaf_surf == 0.0
    assert k2.sizes()[0].tolist() == k.sizes()[0].tolist() and k2.sizes()[1].tolist() == k.sizes()[1].tolist()
    for i in range(3):
        for a, b in zip(k.get(i), k2.get(i)):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(mapio.MapFileError):
        mapio.load_keyframes(path, gpu, keyframes=k)                  # a filtering store would filter the stored lists again
    k.close(); k2.close()
