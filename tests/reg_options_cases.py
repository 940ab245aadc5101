"""The calls whose results tests/golden/reg_options_parent_v1.npz records (tests/golden/make_reg_options_golden.py) and
tests/test_gpu_reg_options.py replays: everything a registration call carries besides its clouds (uncertainty, pose prior, degeneracy
hold, outlier rejection, the SLAM step's map window), through the handle's record sinks and through the SLAM session's slot records.

Every function returns a dict of numpy arrays: raw bytes as uint8, statuses as int32.  Nothing in it depends on the build.
"""
import ctypes as C

import numpy as np

N_SCANS = 6             # scan 0 has no odometry match, scans >= 2 reuse a buffer set, scans >= 4 reuse a slot
MIN_EIG = 150.0         # docs/kernels/uncertainty.md: between a corridor's weak eigenvalue and the next
WINDOW = ((4, 4, 2), 2)  # half_cells, every_n_scans: crops after scans 3 and 5
B = 3


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def _sqrt_info():
    return np.diag([10.0, 10.0, 10.0, 50.0, 50.0, 50.0])


def slam_session(capi, scans, truth, pipelined):
    """Six scans with the features switched mid-session: scans 0-1 everything off; from scan 2 uncertainty, degeneracy for mapping only,
    threshold rejection for odometry and fraction rejection for mapping, a map window every second scan; before scan 3 a next-scan prior
    for the mapping matcher only; before scan 5 rejection cleared.  Per scan: the result record (under the mask of
    tests/test_gpu_pose_prior.py::_rec_core), the four side-record pairs and the status of each of their getters (a refusing getter
    leaves its pair all zero)."""
    from tests.test_gpu_pose_prior import _rec_core
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans[:N_SCANS]), max_rings=16, pose_odom2map=truth[0])
    getters = (("unc", slam.lib.msfl_slam_get_uncertainty, capi.UNCERTAINTY_DTYPE.itemsize),
               ("degen", slam.lib.msfl_slam_get_degeneracy, capi.DEGENERACY_DTYPE.itemsize),
               ("rej", slam.lib.msfl_slam_get_rejection, capi.REJECTION_DTYPE.itemsize),
               ("win", slam.lib.msfl_slam_get_map_window, C.sizeof(capi.GridCropInfo)))
    out = {"rec": [None] * N_SCANS}
    for name, _, _ in getters:
        out[name] = [None] * N_SCANS
        out[name + "_status"] = [None] * N_SCANS

    def fetch(k):
        out["rec"][k] = _u8(_rec_core(slam.result(k)))
        for name, fn, size in getters:
            pair = np.zeros(2 * size, np.uint8)
            out[name + "_status"][k] = fn(slam.s, C.c_int(k), C.c_void_p(pair.ctypes.data), C.c_void_p(pair.ctypes.data + size))
            out[name][k] = pair

    for k in range(N_SCANS):
        if k == 2:
            slam.set_uncertainty(True, MIN_EIG)
            slam.set_degeneracy(odometry=None, mapping=MIN_EIG)
            slam.set_outlier_rejection(odometry=capi.outlier_rejection(threshold=0.2), mapping=capi.outlier_rejection(fraction=0.15))
            slam.set_map_window(*WINDOW)
        if k == 3:
            slam.set_next_prior(odometry=None, mapping=(truth[3], _sqrt_info()))
        if k == 5:
            slam.set_outlier_rejection(None, None)
        slam.add_scan(*scans[k], wait=False)
        if pipelined:
            if k >= 1:
                fetch(k - 1)
        else:
            fetch(k)
    if pipelined:
        fetch(N_SCANS - 1)
    slam.close()
    tag = "slam_pipelined_" if pipelined else "slam_sync_"
    return {tag + name: np.array(v, np.int32) if name.endswith("_status") else np.stack(v) for name, v in out.items()}


def batch_inputs(oracle):
    from tests import common
    cs, ss, guesses, truths = [], [], [], []
    for pts, ring, truth, guess in common.scans(B):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        cs.append(corner); ss.append(surf); guesses.append(guess); truths.append(truth)
    co = np.cumsum([0] + [len(c) for c in cs]).astype(np.int32)
    so = np.cumsum([0] + [len(s) for s in ss]).astype(np.int32)
    return np.concatenate(cs), co, np.concatenate(ss), so, np.array(guesses), np.array(truths)


def batch(capi, oracle, device_sinks):
    """msfl_match_scan2map_batch, B = 3 on common.small_world(), all four features on at once (fraction rejection before every solve):
    poses, status, info and the three record arrays, through host sinks or through device sinks (and device prior records)."""
    import torch
    from tests import common
    _, mc, ms = common.small_world()
    c, co, s, so, guesses, truths = batch_inputs(oracle)
    priors = capi.pose_priors(truths, np.stack([_sqrt_info()] * B))
    kw = dict(fraction=0.15, which=capi.REJECT_EVERY_OUTER)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    if device_sinks:
        dev = torch.device("cuda", 0)
        sink = {name: torch.full((B * dt.itemsize,), 255, dtype=torch.uint8, device=dev)
                for name, dt in (("unc", capi.UNCERTAINTY_DTYPE), ("degen", capi.DEGENERACY_DTYPE), ("rej", capi.REJECTION_DTYPE))}
        d_priors = torch.from_numpy(priors.view(np.uint8).copy()).to(dev)
        torch.cuda.synchronize()
        h.set_uncertainty_device(sink["unc"], B, MIN_EIG)
        h.set_pose_prior_device(d_priors, B)
        h.set_degeneracy_device(MIN_EIG, sink["degen"], B)
        h.set_outlier_rejection_device(sink["rej"], B, **kw)
    else:
        h.set_uncertainty(B, MIN_EIG)
        h.set_pose_prior(truths, np.stack([_sqrt_info()] * B))
        h.set_degeneracy(MIN_EIG, B)
        h.set_outlier_rejection(n=B, **kw)
    poses, status, info = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    h.synchronize()
    if device_sinks:
        recs = {name: t.cpu().numpy() for name, t in sink.items()}
    else:
        recs = {"unc": _u8(h.uncertainty(B).tobytes()), "degen": _u8(h.degeneracy(B).tobytes()), "rej": _u8(h.rejection(B).tobytes())}
    h.close()
    tag = "batch_device_" if device_sinks else "batch_host_"
    out = {tag + "poses": _u8(poses.tobytes()), tag + "status": np.asarray(status, np.int32), tag + "info": _u8(bytes(info))}
    out.update({tag + name: v for name, v in recs.items()})
    return out


# (key prefix, what runs it): one entry per test case of tests/test_gpu_reg_options.py
CASES = ("slam_sync", "slam_pipelined", "batch_host", "batch_device")


def run(capi, oracle, slam_scans, case):
    if case.startswith("slam"):
        _, _, truth, scans = slam_scans
        return slam_session(capi, scans, truth, case == "slam_pipelined")
    return batch(capi, oracle, case == "batch_device")
