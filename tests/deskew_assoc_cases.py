"""Inputs and model of tests/test_gpu_deskew_assoc.py (GPU) and tests/test_deskew_assoc_model.py (CPU): the de-skew association
(knn5_scan2map_kernel<true> + fit_scan2map_kernel<true>, msf_loam_amd/csrc/msfl_kernels.cuh) record by record.

TEST INFRASTRUCTURE.  The model is composed from what is already pinned.  For feature i with time dt_i (the f32 stamp, as f64):

    shift_i  = V dt_i - G dt_i^2 / 2
    full_i.t = R_T (R_T^-1 shift_i + dp_i) + t_T            (mapping_scan_matcher.cc:120 / :190)
    full_i.q = normalized(q_T * dq_i)
    {C, N}   = the plain oracle's association of that ONE feature at pose full_i (oracle.associate_scan2map, exhaustive search,
               a one-point cloud)
    C'       = C - shift_i on accepted features, an all-zero record on rejected ones
    p'_i     = dq_i p_i + dp_i                              numpy f64

Inputs: common.small_world() and two scans' oracle features, each under two motions (below).  The corner list is unvoxelised and,
since one scan of this world yields only ~400 corner features, pooled from POOL scans (each brought into the case's scan frame in
f64: all of them lie on the same map), so that the accepted edge count passes the solve's dense edge list of 1 024.  The motions: the gentle one of
tests/test_gpu_scan2map.py (0.03 rad, 5 mm, 8 cm of velocity shift over the scan) and a strong one (3 rad/s, dp up to 0.2 m, |V| = 15 m/s, G = 9.81).  The raw features are made by
INVERSE distortion, p_raw = dq^-1 (p - dp - R_truth^-1 shift) cast to f32, so that the de-skewed scan lands on the map at the true
pose and most features are accepted.

`model(case, way)` composes the full pose in two ways -- 0: quaternion product and the formula above as written; 1: rotation
matrices (R_T R_dq converted back to a quaternion; t = shift + R_T dp + t_T) -- which differ in the last bits.  A feature whose
accept decision sits on a threshold (the d^2 < 1 gate, the 3 x eigen ratio, the 0.2 m plane check) flips between two such
evaluations; the seeds are chosen so that none does (tests/test_deskew_assoc_model.py), and the GPU's accept set must then be the
model's exactly.
"""
import collections
import functools

import numpy as np

from msf_loam_amd import synth
from tests import common

G = np.array([0.0, 0.0, 9.81])
SCAN_PERIOD = 0.1
POOL = 8                             # scans whose corner features are pooled (one scan's unvoxelised list holds ~400)
Case = collections.namedtuple("Case", "scan motion")
CASES = [Case(s, m) for s in (0, 1) for m in ("gentle", "strong")]
SEEDS = {Case(0, "gentle"): 5101, Case(0, "strong"): 5102, Case(1, "gentle"): 5103, Case(1, "strong"): 5104}

Inputs = collections.namedtuple("Inputs", "corner surf corner_dq corner_dp surf_dq surf_dp V truth guess")


def case_id(c):
    return "scan%d-%s" % (c.scan, c.motion)


def _unit(v):
    return v / np.linalg.norm(v)


def _rotate(dq, p):
    """Row-wise R(dq_i) p_i."""
    return np.stack([synth.quat_to_matrix(q) @ v for q, v in zip(dq, p)]) if len(p) else np.zeros((0, 3))


def _motion(rng, motion):
    """(rotation rate [rad/s], drift of dp [m/s], V [m/s]) of a scan."""
    if motion == "gentle":
        return np.array([0.02, -0.01, 0.3]), np.array([0.05, 0.02, -0.01]), np.array([0.8, -0.3, 0.05])
    rate = 3.0 * _unit(rng.normal(size=3))                                           # 3 rad/s: 0.3 rad at the end of the scan
    drift = 0.2 / SCAN_PERIOD * _unit(rng.normal(size=3))                            # 0.2 m at the end of the scan
    return rate, drift, 15.0 * _unit(rng.normal(size=3))


@functools.lru_cache(maxsize=None)
def inputs(case):
    from oracle import oracle as orc
    orc.build()
    scans = common.scans(POOL)
    pts, ring, truth, guess = scans[case.scan]
    f = orc.extract_features(pts, ring)
    rng = np.random.default_rng(SEEDS[case])
    Rt = synth.quat_to_matrix(truth[3:])
    # the corner features of all POOL scans, brought into this scan's frame (f64): they lie on the same map
    pool = []
    for pts_j, ring_j, truth_j, _ in scans:
        fj = orc.extract_features(pts_j, ring_j)
        cj = fj["full"][fj["less_sharp"]][:, :3].astype(np.float64)
        pool.append((cj @ synth.quat_to_matrix(truth_j[3:]).T + truth_j[:3] - truth[:3]) @ Rt)
    rate, drift, V = _motion(rng, case.motion)
    motions = {}
    for name, p in (("corner", np.concatenate(pool)), ("surf", orc.voxel_grid(f["full"][f["less_flat"]], 0.4)[:, :3].astype(np.float64))):
        t32 = rng.uniform(0.0, SCAN_PERIOD, len(p)).astype(np.float32)
        t = t32.astype(np.float64)
        dq = np.stack([synth.quat_from_rotvec(r) for r in np.outer(t, rate)])
        dp = np.outer(t, drift) + rng.normal(0, 1e-4, (len(t), 3))
        shift = np.outer(t, V) - 0.5 * np.outer(t * t, G)
        conj = dq * np.array([-1.0, -1.0, -1.0, 1.0])
        raw = np.zeros((len(p), 4), np.float32)
        raw[:, :3] = _rotate(conj, p - dp - shift @ Rt).astype(np.float32)           # (shift @ Rt: rows R_truth^-1 shift_i)
        raw[:, 3] = t32
        motions[name] = (raw, dq, dp)
    out = Inputs(motions["corner"][0], motions["surf"][0], motions["corner"][1], motions["corner"][2], motions["surf"][1],
                 motions["surf"][2], V, np.array(truth), np.array(guess))
    for a in out:
        a.setflags(write=False)
    return out


def _quat_from_matrix(R):
    """Shepperd's method, [x y z w] with w >= 0 handled by the caller's comparison (q and -q are one rotation)."""
    tr = np.trace(R)
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def full_pose(pose, dq, dp, shift, way):
    """The per-feature pose of the de-skew association, composed as written (way 0) or through rotation matrices (way 1)."""
    R = synth.quat_to_matrix(pose[3:])
    if way == 0:
        t = R @ (R.T @ shift + dp) + pose[:3]
        q = synth.quat_mul(pose[3:], dq)
        q = q / np.linalg.norm(q)
    else:
        t = shift + R @ dp + pose[:3]
        q = _quat_from_matrix(R @ synth.quat_to_matrix(dq))
    return np.concatenate([t, q])


Model = collections.namedtuple("Model", "accepted rec points")


@functools.lru_cache(maxsize=None)
def model(case, way=0, at="truth"):
    """(accepted (n,) bool, records {C', N} (n, 6), points p' (n, 3)) of the case, corner features first, associated at the true pose
    (`at` = "truth") or at the scan's perturbed guess ("guess")."""
    from oracle import oracle as orc
    orc.build()
    _, mc, ms = common.small_world()
    x = inputs(case)
    pose = x.truth if at == "truth" else x.guess
    empty = np.zeros((0, 4), np.float32)
    acc, rec, pts = [], [], []
    for cloud, dqs, dps, is_corner in ((x.corner, x.corner_dq, x.corner_dp, True), (x.surf, x.surf_dq, x.surf_dp, False)):
        for f, dq, dp in zip(cloud, dqs, dps):
            dt = float(f[3])
            shift = x.V * dt - 0.5 * G * dt * dt
            one = f.reshape(1, 4)
            c = orc.associate_scan2map(mc, ms, one if is_corner else empty, empty if is_corner else one,
                                       full_pose(pose, dq, dp, shift, way), use_kdtree=False)[0]
            ok = int(c["kind"]) != 0
            acc.append(ok)
            rec.append(np.concatenate([c["C"] - shift, c["N"]]) if ok else np.zeros(6))
            pts.append(synth.quat_to_matrix(dq) @ f[:3].astype(np.float64) + dp)
    out = Model(np.array(acc, bool), np.array(rec).reshape(-1, 6), np.array(pts).reshape(-1, 3))
    for a in out:
        a.setflags(write=False)
    return out
