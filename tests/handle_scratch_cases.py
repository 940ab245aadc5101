"""The calls whose results tests/golden/handle_scratch_parent_v1.npz records (tests/golden/make_handle_scratch_golden.py) and
tests/test_gpu_handle_scratch.py replays: ONE handle driven through every host-memory call that stages through the handle's scratch
(extraction, voxel filters, per-point passes, scan-to-scan, scan-to-map, pairs, scoring) and one Places object, three times over: at
small sizes, at about three times those sizes (every scratch buffer regrows, which drops its contents) and at the small sizes again.
Then the forms of the voxel filter the sequence does not reach: the one-workgroup big form (a 70 000-point cloud), the device-wide
form (a handle created under MSFL_VOXEL_GLOBAL=1) and the pair form on device memory.

A wrongly mapped scratch buffer does not show in a per-feature test; it shows when two features share a handle, or when a buffer
regrows between two calls that expect its contents.

run() returns a dict of numpy arrays: counts, statuses and poses in full, every large array as its SHA-1 digest (20 bytes).  Nothing
in it depends on the build; every input is seeded.
"""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

from msf_loam_amd import synth

ROUNDS = (("r0_small", 1), ("r1_large", 3), ("r2_small", 1))
SCAN_AZ = {1: 160, 3: 480}            # azimuth steps of the 16-beam scans: about 2 000 / 6 000 points
ODOM_AZ = {1: 600, 3: 1800}           # ... of the scans of the scan-to-scan batch: long enough for the column-grid path
MAP_TARGET = {1: 20000, 3: 60000}     # points of the world's map
N_PAIRS = 3
N_HYPOTHESES = 4
BIG_CLOUD = 70000                     # 65 536 .. 131 071 points: the one-workgroup big voxel form
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha1(a.tobytes()).digest(), np.uint8).copy()


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def inputs(scale):
    """Everything a round reads that does not come out of an earlier call of the round."""
    from tests import common
    w, mc, ms = common.small_world(MAP_TARGET[scale])
    poses = synth.random_poses(8, synth.SEED + 40 + scale)
    rng = np.random.default_rng(synth.SEED + 50 + scale)
    at = [poses[0], poses[1], synth.perturb_pose(poses[1], rng, 0.25, 2.0), poses[3]]        # scans 1 and 2 are a scan-to-scan pair
    scans = [synth.make_scan(w, at[i], synth.SEED + 60 + 10 * scale + i, n_az=SCAN_AZ[scale]) for i in range(4)]
    # a slow drive for the scan-to-scan pairs: scan i + 1 a quarter of a metre and two degrees from scan i
    drive = [poses[4]]
    for i in range(3):
        drive.append(synth.perturb_pose(drive[-1], rng, 0.25, 2.0))
    odom = [synth.make_scan(w, drive[i], synth.SEED + 80 + 10 * scale + i, n_az=ODOM_AZ[scale]) for i in range(4)]
    # a scan's worth of IMU pre-integration: constant body rate and acceleration, irregular sample times
    t = np.sort(np.concatenate([[0.0, 0.1], rng.uniform(0, 0.1, 43)]))
    dq = np.array([synth.quat_from_rotvec(np.array([0.02, -0.01, 0.05]) * (x / 0.1)) for x in t])
    dp = np.array([0.03, 0.01, 0.0])[None, :] * (t[:, None] / 0.1) ** 2
    guesses = np.array([synth.perturb_pose(drive[0], rng, 0.2, 2.0) for _ in range(N_HYPOTHESES)])     # of the first scan of the drive
    return dict(world=w, mc=mc, ms=ms, poses=poses, scans=scans, odom=odom, pre=(t, dq, dp), guesses=guesses)


def _timed(pts):
    """The cloud with relative times spread over the pre-integration span."""
    c = np.array(pts, np.float32).reshape(-1, 4).copy()
    c[:, 3] = np.linspace(0.0, 0.0999, len(c), dtype=np.float32)
    return c


def _features(out, tag, f):
    out[tag + "_rc"] = np.array([f["rc"]], np.int32)
    out[tag + "_counts"] = np.array([len(f[k]) for k in ("full", "sharp", "less_sharp", "flat", "less_flat")], np.int32)
    for k in ("full", "ring", "curvature", "label", "sharp", "less_sharp", "flat", "less_flat"):
        out[tag + "_" + k] = digest(f[k])


def _odom_clouds(fa, fb):
    return (fa["full"][fa["less_sharp"]], fa["ring"][fa["less_sharp"]], fa["full"][fa["less_flat"]], fa["ring"][fa["less_flat"]],
            fb["full"][fb["sharp"]], fb["full"][fb["flat"]])


def _batch_sets(pairs):
    sets = []
    for k in range(4):
        pick = lambda p: (p[0], p[2], p[4], p[5])[k]
        pts = np.concatenate([pick(p) for p in pairs])
        off = np.cumsum([0] + [len(pick(p)) for p in pairs]).astype(np.int32)
        ring = np.concatenate([(p[1], p[3])[k] for p in pairs]) if k < 2 else None
        sets.append((pts, ring, off))
    return sets


def one_round(capi, h, places, tag, scale):
    """The interleaved sequence on handle `h` and Places object `places`."""
    x = inputs(scale)
    out = {}
    put = lambda k, v: out.__setitem__(tag + "_" + k, v)
    # ---- extraction: one scan (with an extrinsic: it is staged through the registration's pose buffer), then a batch of three
    f0 = h.extract_features(*x["scans"][0], extrinsic=np.array([0.1, -0.05, 0.2, 0, 0, 0, 1.0]))
    _features(out, tag + "_ex1", f0)
    pts3 = np.concatenate([p for p, _ in x["scans"][1:4]])
    ring3 = np.concatenate([r for _, r in x["scans"][1:4]])
    off3 = np.cumsum([0] + [len(p) for p, _ in x["scans"][1:4]]).astype(np.int32)
    fb = h.extract_features_batch(pts3, ring3, off3)
    for b, f in enumerate(fb):
        _features(out, tag + "_ex3_%d" % b, f)
    # ---- voxel filter: a cloud with a few non-finite points (the compaction of the per-point scratch, then the filter again), a batch
    holed = f0["full"].copy()
    holed[[5, len(holed) // 2, len(holed) - 3], 0] = np.nan
    v = h.voxel_downsample(holed, 0.3)
    put("vox_nan_n", np.array([len(v)], np.int32)); put("vox_nan", digest(v))
    fulls = np.concatenate([f["full"] for f in fb])
    foff = np.cumsum([0] + [len(f["full"]) for f in fb]).astype(np.int32)
    vb, vb_off = h.voxel_downsample_batch(fulls, foff, 0.4)
    put("vox_batch_off", np.asarray(vb_off, np.int32)); put("vox_batch", digest(vb))
    # ---- per-point passes
    t, dq, dp = x["pre"]
    cloud = _timed(f0["full"])
    s, pq, pp = h.delta_qp(t, dq, dp, cloud)
    put("delta_qp_status", np.array([s], np.int32)); put("delta_q", digest(pq)); put("delta_p", digest(pp))
    vel, grav = np.array([0.3, 0.1, 0.0]), np.array([0.0, 0.0, 9.8])
    s, dk = h.deskew_cloud(t, dq, dp, cloud, np.array([0.0, 0.0, 0.1, 0.995]), vel, grav)
    put("deskew_status", np.array([s], np.int32)); put("deskew", digest(dk))
    s, un = h.undistort_cloud(t, dq, dp, cloud)
    put("undistort_status", np.array([s], np.int32)); put("undistort", digest(un))
    put("transform", digest(h.transform_cloud(cloud, x["poses"][0])))
    # ---- scan-to-scan: one small pair (one wavefront per query), then three long pairs (the column-grid path)
    s, pose, info = h.match_scan2scan(*_odom_clouds(fb[0], fb[1]), IDENT)
    put("s2s_status", np.array([s], np.int32)); put("s2s_pose", pose.copy()); put("s2s_info", _u8(info))
    po = np.concatenate([p for p, _ in x["odom"]])
    ro = np.concatenate([r for _, r in x["odom"]])
    oo = np.cumsum([0] + [len(p) for p, _ in x["odom"]]).astype(np.int32)
    fo = h.extract_features_batch(po, ro, oo)
    pairs = [_odom_clouds(fo[i], fo[i + 1]) for i in range(3)]
    targets = sum(len(p[0]) + len(p[2]) for p in pairs)
    assert targets > 4096 * len(pairs), ("the batch would take the one-wavefront-per-query kernel", targets)
    poses, status, info = h.match_scan2scan_batch(_batch_sets(pairs), np.stack([IDENT] * 3), want_info=True)
    put("s2s_batch_status", np.asarray(status, np.int32)); put("s2s_batch_poses", poses.copy()); put("s2s_batch_info", _u8(info))
    # ---- scan-to-map and what goes with it
    corner = h.voxel_downsample(fo[0]["full"][fo[0]["less_sharp"]], 0.2)         # the features of the first scan of the drive
    surf = h.voxel_downsample(fo[0]["full"][fo[0]["less_flat"]], 0.4)
    put("feat_n", np.array([len(corner), len(surf)], np.int32)); put("feat_corner", digest(corner)); put("feat_surf", digest(surf))
    guess = x["guesses"][0]
    h.set_map(x["mc"], x["ms"])
    s, pose, info = h.match_scan2map(corner, surf, guess)
    put("s2m_status", np.array([s], np.int32)); put("s2m_pose", pose.copy()); put("s2m_info", _u8(info))
    ct, st_ = _timed(corner), _timed(surf)
    s1, cq, cp = h.delta_qp(t, dq, dp, ct)
    s2, sq, sp = h.delta_qp(t, dq, dp, st_)
    s, pose, info = h.match_scan2map_deskew(ct, st_, cq, cp, sq, sp, vel, grav, guess)
    put("s2m_deskew_status", np.array([s1, s2, s], np.int32)); put("s2m_deskew_pose", pose.copy()); put("s2m_deskew_info", _u8(info))
    rec = h.associate_scan2map(corner, surf, guess)
    put("assoc_records", digest(rec))
    pose, info = h.solve_records(corner, surf, rec, guess)
    put("solve_pose", pose.copy()); put("solve_info", _u8(info))
    # ---- pairs with maps of their own: the whole map, every second point of it, and a map too small to match against
    maps_c, maps_s = [x["mc"], x["mc"][::2], x["mc"][:4]], [x["ms"], x["ms"][::2], x["ms"][:4]]
    mco = np.cumsum([0] + [len(m) for m in maps_c]).astype(np.int32)
    mso = np.cumsum([0] + [len(m) for m in maps_s]).astype(np.int32)
    co = (np.arange(N_PAIRS + 1) * len(corner)).astype(np.int32)
    so = (np.arange(N_PAIRS + 1) * len(surf)).astype(np.int32)
    poses, status, info = h.match_pairs_batch(np.concatenate(maps_c), mco, np.concatenate(maps_s), mso, np.concatenate([corner] * N_PAIRS), co,
                                              np.concatenate([surf] * N_PAIRS), so, x["guesses"][:N_PAIRS], want_info=True)
    put("pairs_status", np.asarray(status, np.int32)); put("pairs_poses", poses.copy()); put("pairs_info", _u8(info))
    # ---- scoring against the resident map (the pairs call replaced it)
    h.set_map(x["mc"], x["ms"])
    rec, d2, nn = h.score_poses(corner, surf, x["guesses"], 0.8, want_nn=True)
    put("score_records", _u8(rec.tobytes())); put("score_d2", digest(d2)); put("score_nn", digest(nn))
    # ---- place recognition: four scans in, two queries
    first = places.add([p for p, _ in x["scans"]])
    m = places.query([x["scans"][2][0], x["odom"][1][0]], k=3)
    put("place_first", np.array([first, places.size()], np.int32)); put("place_matches", _u8(m.tobytes()))
    return out


def main_handle(capi):
    h = capi.Handle(0)
    places = capi.Places(0, capacity=64)
    out = {}
    try:
        for tag, scale in ROUNDS:
            out.update(one_round(capi, h, places, tag, scale))
        # the one-workgroup big form, on the same handle, and the LDS form after it
        from tests.test_gpu_extract import _sweep_cloud
        big = _sweep_cloud(np.random.default_rng(91), BIG_CLOUD)
        v = h.voxel_downsample(big, 0.4)
        out["big_n"] = np.array([len(v)], np.int32); out["big"] = digest(v)
        v = h.voxel_downsample(big[:3000], 0.4)
        out["after_big_n"] = np.array([len(v)], np.int32); out["after_big"] = digest(v)
    finally:
        places.close()
        h.close()
    return out


def global_voxel(capi):
    """The device-wide voxel form: a handle created under MSFL_VOXEL_GLOBAL=1; one cloud, a batch with an index list, a cloud with NaNs."""
    x = inputs(1)
    old = os.environ.get("MSFL_VOXEL_GLOBAL")
    os.environ["MSFL_VOXEL_GLOBAL"] = "1"
    try:
        h = capi.Handle(0)
    finally:
        if old is None:
            del os.environ["MSFL_VOXEL_GLOBAL"]
        else:
            os.environ["MSFL_VOXEL_GLOBAL"] = old
    out = {}
    try:
        clouds = [p for p, _ in x["scans"][:3]]
        v = h.voxel_downsample(clouds[0], 0.3)
        out["global_one_n"] = np.array([len(v)], np.int32); out["global_one"] = digest(v)
        off = np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)
        rng = np.random.default_rng(7)
        idx = np.concatenate([rng.permutation(len(c)).astype(np.int32) for c in clouds])
        cnt = np.array([len(c) // 2 for c in clouds], np.int32)
        v, voff = h.voxel_downsample_batch(np.concatenate(clouds), off, 0.4, idx=idx, count=cnt)
        out["global_batch_off"] = np.asarray(voff, np.int32); out["global_batch"] = digest(v)
        holed = clouds[1].copy()
        holed[[0, 77, len(holed) - 1], 1] = np.inf
        v = h.voxel_downsample(holed, 0.3)
        out["global_nan_n"] = np.array([len(v)], np.int32); out["global_nan"] = digest(v)
    finally:
        h.close()
    return out


def pair_device(capi):
    """msfl_voxel_downsample_batch_pair on device memory, B = 2: both lists through the LDS form, list a in the pair's own scratch set."""
    import torch
    x = inputs(1)
    dev = torch.device("cuda", 0)
    clouds = [p for p, _ in x["scans"][:2]]
    B = len(clouds)
    off = np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)
    n = int(off[-1])
    rng = np.random.default_rng(9)
    idx = [np.concatenate([rng.permutation(len(c)).astype(np.int32) for c in clouds]) for _ in range(2)]
    cnt = [np.array([len(c) // 2 for c in clouds], np.int32), np.array([len(c) - 10 for c in clouds], np.int32)]
    d_pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_idx = [torch.from_numpy(a).to(dev) for a in idx]
    d_cnt = [torch.from_numpy(a).to(dev) for a in cnt]
    d_out = [torch.zeros((n, 4), dtype=torch.float32, device=dev) for _ in range(2)]
    oo = [np.zeros(B + 1, np.int32) for _ in range(2)]
    torch.cuda.synchronize()
    vp = C.c_void_p
    h = capi.Handle(0)
    out = {}
    try:
        s = h.lib.msfl_voxel_downsample_batch_pair(h.h, C.c_int(B), vp(d_pts.data_ptr()), off.ctypes.data_as(vp),
                                                   vp(d_idx[0].data_ptr()), vp(d_cnt[0].data_ptr()), C.c_float(0.2), vp(d_out[0].data_ptr()), oo[0].ctypes.data_as(vp),
                                                   vp(d_idx[1].data_ptr()), vp(d_cnt[1].data_ptr()), C.c_float(0.4), vp(d_out[1].data_ptr()), oo[1].ctypes.data_as(vp),
                                                   C.c_int(capi.MEM_DEVICE))
        h.synchronize()
        out["pair_status"] = np.array([s], np.int32)
        for k, name in enumerate("ab"):
            out["pair_off_" + name] = oo[k].copy()
            out["pair_out_" + name] = digest(d_out[k][:int(oo[k][-1])].cpu().numpy())
        # the single-list call on the same handle afterwards: it shares list b's scratch set
        v, voff = h.voxel_downsample_batch(np.concatenate(clouds), off, 0.4)
        out["pair_then_batch_off"] = np.asarray(voff, np.int32); out["pair_then_batch"] = digest(v)
    finally:
        h.close()
    return out


def check_coverage(got, capi):
    """What the sequence is for, read off its results (no GPU needed): every call succeeded except the pair whose map is too small, the
    third round on the regrown buffers repeats the first byte for byte (the Places database alone has grown in between), and every
    voxel form delivered something."""
    for key, v in got.items():
        if key.endswith("_status") and "pairs" not in key:
            assert not v.any(), (key, v.tolist())
        if key.endswith("_rc"):
            assert not v.any(), (key, v.tolist())
    for tag, _ in ROUNDS:
        assert got[tag + "_pairs_status"].tolist() == [capi.OK, capi.OK, capi.MAP_TOO_SMALL], tag
        assert got[tag + "_vox_nan_n"][0] > 0 and got[tag + "_feat_n"].min() > 20 and np.diff(got[tag + "_vox_batch_off"]).min() > 0, tag
    first, last = ROUNDS[0][0], ROUNDS[2][0]
    for key in got:
        if key.startswith(first + "_") and "_place_" not in key:
            assert got[key].tobytes() == got[last + key[len(first):]].tobytes(), key
    assert got[first + "_place_first"].tolist() == [0, 4] and got[last + "_place_first"].tolist() == [8, 12]
    assert got["big_n"][0] > 0 and got["after_big_n"][0] > 0 and got["global_one_n"][0] > 0 and got["global_nan_n"][0] > 0
    assert got["pair_status"][0] == 0 and got["pair_off_a"][-1] > 0 and got["pair_off_b"][-1] > 0


def run(capi):
    out = main_handle(capi)
    out.update(global_voxel(capi))
    out.update(pair_device(capi))
    return out
