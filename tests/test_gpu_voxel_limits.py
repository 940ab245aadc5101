"""GPU: the voxel filter (pcl::VoxelGrid, bit for bit) at the structural limits of its four forms.

The cases are tests/voxel_limit_cases.py's; tests/test_voxel_form_model.py proves on the CPU that each one sits on the side of its
edge that its name claims.  Here every case runs on three handles -- the default one, MSFL_VOXEL_NO_BIG=1 (no big one-workgroup
form: what the LDS forms refuse goes to the device-wide form) and MSFL_VOXEL_GLOBAL=1 (the device-wide form alone) -- and every
cloud must equal oracle.voxel_grid AS BIT PATTERNS (np.array_equal takes -0.0 for +0.0), with equal offsets, on all three.  There
is no tolerance anywhere in this file.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import voxel_limit_cases as vc

pytestmark = pytest.mark.gpu

HANDLES = ("default", "no_big", "global")


@pytest.fixture(scope="module")
def handles():
    from msf_loam_amd import capi
    saved = {k: os.environ.pop(k, None) for k in ("MSFL_VOXEL_NO_BIG", "MSFL_VOXEL_GLOBAL")}
    hs = {}
    try:
        hs["default"] = capi.Handle(0)
        os.environ["MSFL_VOXEL_NO_BIG"] = "1"; hs["no_big"] = capi.Handle(0); del os.environ["MSFL_VOXEL_NO_BIG"]
        os.environ["MSFL_VOXEL_GLOBAL"] = "1"; hs["global"] = capi.Handle(0); del os.environ["MSFL_VOXEL_GLOBAL"]
        yield hs
    finally:
        for h in hs.values():
            h.close()
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=4)
def _reference(name):
    """The oracle's result per cloud of a case (None for the cloud a T / X case has refused), computed once."""
    from oracle import oracle as orc
    orc.build()
    c = vc.case(name)
    refs = []
    for b, cloud in enumerate(c.clouds):
        refused = c.status != "OK" and b == c.target
        refs.append(None if refused else orc.voxel_grid(cloud, c.leaf) if len(cloud) else np.zeros((0, 4), np.float32))
    return refs


def _scatter(name, c):
    """The case's clouds stored scattered, each in a region with slack, and listed in cloud order through idx / count."""
    rng = np.random.default_rng(len(name))
    clouds = c.clouds
    off = np.cumsum([0] + [len(cl) + 29 for cl in clouds]).astype(np.int32)
    full = np.zeros((off[-1], 4), np.float32); idx = np.zeros(off[-1], np.int32)
    for b, cl in enumerate(clouds):
        perm = rng.permutation(len(cl) + 29)[:len(cl)]
        full[off[b] + perm] = cl; idx[off[b]:off[b] + len(cl)] = perm
    return full, off, idx, np.array([len(cl) for cl in clouds], np.int32)


def _batch(h, pts, off, leaf, idx=None, count=None):
    """msfl_voxel_downsample_batch on host memory -> (status, out, out_off): unlike Handle.voxel_downsample_batch it hands back
    what a refusing call has delivered."""
    off = np.ascontiguousarray(off, np.int32)
    B = len(off) - 1
    out = np.full((max(int(off[-1] - off[0]), 1), 4), np.nan, np.float32)
    out_off = np.full(B + 1, -1, np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s = h.lib.msfl_voxel_downsample_batch(h.h, C.c_int(B), vp(pts), vp(idx), vp(off), vp(count), C.c_float(leaf), vp(out), vp(out_off), C.c_int(0))
    return s, out, out_off


def _check_delivered(tag, out, out_off, refs):
    """Offsets and every delivered cloud against the oracle; a refused cloud (ref None) has an empty range."""
    want = np.r_[0, np.cumsum([0 if r is None else len(r) for r in refs])]
    assert np.array_equal(out_off, want), (tag, out_off[:8], want[:8])
    for b, r in enumerate(refs):
        if r is not None:
            got = out[out_off[b]:out_off[b + 1]]
            assert _same(got, r), (tag, b, len(r), int((_bits(got) != _bits(r)).any(axis=1).sum()) if got.shape == r.shape else got.shape)


@pytest.mark.parametrize("name", [n for n in vc.NAMES if n not in vc.REFUSED and n[0] != "Q"])
def test_case_equals_the_oracle_bit_for_bit_on_every_form(handles, name):
    from msf_loam_amd import capi
    c = vc.case(name)
    refs = _reference(name)
    assert len(refs[c.target]) == c.voxels
    outs = {}
    for k in HANDLES:
        h = handles[k]
        if c.scattered:
            full, off, idx, cnt = _scatter(name, c)
            s, out, out_off = _batch(h, full, off, c.leaf, idx, cnt)
        else:
            s, out, out_off = _batch(h, c.pts, c.off, c.leaf)
        assert s == capi.OK, (k, s, h.lib.msfl_last_error(h.h))
        _check_delivered((name, k), out, out_off, refs)
        outs[k] = (out[:out_off[-1]], out_off)
        if name in vc.SINGLE:
            assert _same(h.voxel_downsample(c.pts, c.leaf), refs[0]), (name, k, "msfl_voxel_downsample")
    for k in HANDLES[1:]:
        assert _same(outs[k][0], outs["default"][0]) and np.array_equal(outs[k][1], outs["default"][1]), k


@pytest.mark.parametrize("name", vc.REFUSED)
def test_leaf_too_small_is_capacity_for_that_cloud_alone(handles, name):
    """T: more than 2^31 - 1 cells; X: a voxel coordinate no int holds.  On every form the call returns MSFL_CAPACITY, the refused
    cloud's output range is empty, the clouds around it are delivered, and the handle's next call is right."""
    from msf_loam_amd import capi
    c = vc.case(name)
    refs = _reference(name)
    assert refs[c.target] is None and all(r is not None and len(r) for b, r in enumerate(refs) if b != c.target)
    for k in HANDLES:
        h = handles[k]
        s, out, out_off = _batch(h, c.pts, c.off, c.leaf)
        print(name, k, "status", s, "out_off", out_off)
        assert s == capi.CAPACITY, (name, k, s)
        _check_delivered((name, k), out, out_off, refs)
        target = np.ascontiguousarray(c.clouds[c.target])                                   # alone, through both entry points
        s1, _, oo1 = _batch(h, target, np.array([0, len(target)], np.int32), c.leaf)
        assert s1 == capi.CAPACITY and oo1[1] == 0, (name, k, s1, oo1)
        with pytest.raises(capi.MsflError) as e:
            h.voxel_downsample(target, c.leaf)
        assert e.value.status == capi.CAPACITY
        first = np.ascontiguousarray(c.clouds[0])                                           # the next ordinary call
        assert _same(h.voxel_downsample(first, c.leaf), refs[0]), (name, k, "the call after the refusal")


@pytest.mark.parametrize("name", ["T_1291_S", "T_1291_L", "T_1291_B"])
@pytest.mark.parametrize("refused_list", ["a", "b"])
def test_pair_call_refuses_one_list_and_delivers_the_other(gpu, oracle, name, refused_list):
    """msfl_voxel_downsample_batch_pair on device memory: the cloud whose leaf is too small is in one list only.  MSFL_CAPACITY,
    that list's range for the cloud is empty and its other clouds are delivered; the other list is what it is without it."""
    import torch
    from msf_loam_amd import capi
    dev = torch.device("cuda", 0)
    c = vc.case(name)
    clouds = c.clouds
    other = vc.points_in(np.random.default_rng(5), vc.sweep(1200, 4, (12, 12, 12), (-6, -6, -6)), 0.5)
    regions = [clouds[0], np.concatenate([clouds[1], other]), clouds[2]]
    off = np.cumsum([0] + [len(r) for r in regions]).astype(np.int32)
    n, n_t = int(off[-1]), len(clouds[1])
    full = np.ascontiguousarray(np.concatenate(regions), np.float32)
    lists = {"t": ([np.arange(len(clouds[0])), np.arange(n_t), np.arange(len(clouds[2]))], c.leaf),            # holds the refused cloud
             "o": ([np.arange(len(clouds[0])), n_t + np.arange(len(other)), np.arange(len(clouds[2]))], 0.5)}    # ordinary clouds only
    idx, cnt, leaf, refs = {}, {}, {}, {}
    for key, (ls, lf) in lists.items():
        idx[key] = np.zeros(n, np.int32); cnt[key] = np.array([len(l) for l in ls], np.int32); leaf[key] = lf
        for b, l in enumerate(ls):
            idx[key][off[b]:off[b] + len(l)] = l
        refs[key] = [None if (key == "t" and b == 1) else oracle.voxel_grid(regions[b][l], lf) for b, l in enumerate(ls)]
    order = ("t", "o") if refused_list == "a" else ("o", "t")
    t = lambda a: torch.from_numpy(a).to(dev)
    d_full = t(full)
    d_idx = [t(idx[k]) for k in order]; d_cnt = [t(cnt[k]) for k in order]
    outs = [torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    oo = [np.full(4, -1, np.int32) for _ in range(2)]
    vp = C.c_void_p
    s = gpu.lib.msfl_voxel_downsample_batch_pair(gpu.h, C.c_int(3), vp(d_full.data_ptr()), off.ctypes.data_as(vp),
                                                 vp(d_idx[0].data_ptr()), vp(d_cnt[0].data_ptr()), C.c_float(leaf[order[0]]), vp(outs[0].data_ptr()), oo[0].ctypes.data_as(vp),
                                                 vp(d_idx[1].data_ptr()), vp(d_cnt[1].data_ptr()), C.c_float(leaf[order[1]]), vp(outs[1].data_ptr()), oo[1].ctypes.data_as(vp),
                                                 C.c_int(capi.MEM_DEVICE))
    assert s == capi.CAPACITY, s
    for i, key in enumerate(order):
        _check_delivered((name, refused_list, key), outs[i].cpu().numpy(), oo[i], refs[key])
    assert _same(gpu.voxel_downsample(np.ascontiguousarray(clouds[0]), c.leaf), refs["t"][0])


@pytest.mark.parametrize("name", list(vc.Q_SPEC))
def test_the_device_wide_key_at_64_and_65_bits(handles, oracle, name):
    """65 536 / 65 537 clouds of one point each but one, which spans 1100^3 cells: on the MSFL_VOXEL_GLOBAL handle 64 key bits
    (the run number in the key's low bits) and 65 (the (key, value) sort); on the default one every cloud takes S.  A one-point
    cloud's centroid is (0 + x) / 1 = x for the non-zero coordinates the case has, so those are compared with the input itself,
    and a sample of them with the oracle as well.  The `revisit` case swaps one of them for a cloud with a voxel visited three
    times: with 65 key bits nothing but the stability of the (key, value) sort keeps that voxel's runs in arrival order."""
    from msf_loam_amd import capi
    c = vc.case(name)
    B = len(c.off) - 1
    two = oracle.voxel_grid(c.clouds[c.target], c.leaf)
    assert len(two) == 2 and (c.pts != 0).all()
    more = {c.target: two}
    if vc.Q_SPEC[name][1]:
        # a voxel visited three times, whose centroid differs in every lane when its runs are summed in another order: with 65 key
        # bits only the stability of the (key, value) sort keeps them in arrival order
        more[vc.Q_REVISIT_CLOUD] = oracle.voxel_grid(c.clouds[vc.Q_REVISIT_CLOUD], c.leaf)
        assert len(more[vc.Q_REVISIT_CLOUD]) == 3
    sizes = np.ones(B, np.int64)
    want = c.pts.copy()
    for b in sorted(more, reverse=True):
        want = np.concatenate([want[:c.off[b]], more[b], want[c.off[b + 1]:]]); sizes[b] = len(more[b])
    want_off = np.r_[0, np.cumsum(sizes)]
    for b in list(range(0, B, 1021)) + [c.target - 1, c.target + 1, B - 1]:
        assert _same(oracle.voxel_grid(c.clouds[b], c.leaf), want[want_off[b]:want_off[b + 1]])
    for k in ("global", "default"):
        s, out, out_off = _batch(handles[k], c.pts, c.off, c.leaf)
        assert s == capi.OK, (k, s)
        assert np.array_equal(out_off, want_off), k                                   # every one-point cloud keeps its size
        bad = np.flatnonzero((_bits(out[:len(want)]) != _bits(want)).any(axis=1))
        assert len(bad) == 0, (k, len(bad), bad[:8])
