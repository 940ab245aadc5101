"""The batches of tests/test_gpu_record_tiles.py and how they are run (shared with tests/golden/make_record_tiles_golden.py, which
records the same runs from the library of the commit before the record tiles).

The plane records of a batch live in lane-transposed tiles of 64 rows (msf_loam_amd/csrc/msfl_record_tiles.h) and, on the
whole-batch path, a surf feature's 5-NN list is kept in the tile its record will occupy.  Neither may change one bit of a result,
so every run below is compared bit for bit with what the row-major layout gave.

Batch A -- 14 scans, surf clouds at a 0.1 m leaf (~14 000 surf features per scan).  It is sized so that BOTH parts of the chunked
host-buffer call (7 scans each, one of them without surf features) still hold >= 65 536 records and take the whole-batch kernels in
their second pass; 14 scans of ~5 000 features (the smallest whole-batch batch) would fall below the threshold once split in two.
Every scan is cut to a surf count of its own so that the scans' first plane slots fall into 13 different residue classes mod 64
(the scan after the one without surf features shares its start), the last tile is partial, and both clouds start at a non-zero
offset of their arrays.  One scan has no surf features, one no corner features.

Batch B -- 3 scans with surf counts (130, 64, 61) and corner counts (0, 7, 70): the per-record kernels, scans that start mid-tile,
a scan that is exactly one tile.
"""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

from msf_loam_amd import synth
from tests import common

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_tiles_parent_v1.npz")

A_SCANS = 14
A_NO_SURF, A_NO_CORNER, A_BAD_PRIOR = 3, 9, 6
# first plane slot of scan i mod 64 (scan A_NO_SURF + 1 starts where A_NO_SURF does), then where the batch ends: a partial last tile
A_RESIDUES = (0, 1, 63, 32, 32, 5, 47, 33, 62, 2, 21, 40, 9, 58, 13)
A_C0, A_S0 = 5, 77                       # corner_off[0], surf_off[0]
A_PART_SCANS = 7                         # MSFL_H2D_CHUNK_SCANS of the chunked run: two parts
B_SURF, B_CORNER = (130, 64, 61), (0, 7, 70)
B_REJECT_THRESHOLD = 0.05                # metres: rejects planes mid-tile (the generator checks that some are)

FIELDS = ("poses", "status", "n_edge", "n_plane", "lm_iterations", "initial_cost", "final_cost")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def result(poses, status, info):
    """What a run is compared by: poses and costs as f64 bit patterns, status, per-iteration correspondence and LM iteration counts."""
    return {"poses": _bits(np.asarray(poses).reshape(-1, 7)),
            "status": np.asarray(status, np.int32).reshape(-1),
            "n_edge": np.array([list(r.n_edge) for r in info], np.int32),
            "n_plane": np.array([list(r.n_plane) for r in info], np.int32),
            "lm_iterations": np.array([list(r.lm_iterations) for r in info], np.int32),
            "initial_cost": _bits(np.array([list(r.initial_cost) for r in info])),
            "final_cost": _bits(np.array([list(r.final_cost) for r in info]))}


@functools.lru_cache(maxsize=None)
def _features(orc, surf_leaf):
    out = []
    for pts, ring, truth, _ in common.scans(6):
        f = orc.extract_features(pts, ring)
        out.append((orc.voxel_grid(f["full"][f["less_sharp"]], 0.2), orc.voxel_grid(f["full"][f["less_flat"]], surf_leaf), truth))
    return out


@functools.lru_cache(maxsize=None)
def batch_a(orc):
    """(corner array, corner_off, surf array, surf_off, guesses): the arrays begin with A_C0 / A_S0 points that belong to no scan."""
    feats = _features(orc, 0.1)
    rng = np.random.default_rng(8101)
    cs, ss, gs = [], [], []
    for i in range(A_SCANS):
        c, s, truth = feats[i % 6]
        want = (A_RESIDUES[i + 1] - A_RESIDUES[i]) % 64
        n = 0 if i == A_NO_SURF else len(s) - (len(s) - want) % 64 - 64 * i          # a different count for every scan
        cs.append(c[:0] if i == A_NO_CORNER else c); ss.append(s[:n]); gs.append(synth.perturb_pose(truth, rng))
    co = (A_C0 + np.cumsum([0] + [len(c) for c in cs])).astype(np.int32)
    so = (A_S0 + np.cumsum([0] + [len(s) for s in ss])).astype(np.int32)
    starts = (so - A_S0) % 64
    assert tuple(int(x) for x in starts) == A_RESIDUES and len(set(A_RESIDUES[:A_SCANS])) == A_SCANS - 1
    assert len({len(s) for s in ss}) == A_SCANS
    for b0, b1 in ((0, A_PART_SCANS), (A_PART_SCANS, A_SCANS)):              # each part of the chunked run: the whole-batch threshold
        assert (co[b1] - co[b0]) + (so[b1] - so[b0]) >= 65536
    junk = np.full((A_S0, 4), 1.0e3, np.float32)
    C_ = np.ascontiguousarray(np.concatenate([junk[:A_C0]] + cs), np.float32)
    S_ = np.ascontiguousarray(np.concatenate([junk] + ss), np.float32)
    return C_, co, S_, so, np.array(gs, np.float64)


@functools.lru_cache(maxsize=None)
def batch_b(orc):
    feats = _features(orc, 0.4)
    rng = np.random.default_rng(8102)
    cs, ss, gs = [], [], []
    for i, (ns, nc) in enumerate(zip(B_SURF, B_CORNER)):
        c, s, truth = feats[i]
        cs.append(c[:: max(1, len(c) // max(nc, 1))][:nc]); ss.append(s[:: len(s) // ns][:ns]); gs.append(synth.perturb_pose(truth, rng))
        assert len(cs[-1]) == nc and len(ss[-1]) == ns
    return cs, ss, np.array(gs, np.float64)


def inputs_digest(orc):
    """sha256 over every input array: the fixture is only valid for these bytes."""
    h = hashlib.sha256()
    _, mc, ms = common.small_world()
    for a in (mc, ms) + tuple(batch_a(orc)) + tuple(batch_b(orc)[0]) + tuple(batch_b(orc)[1]) + (batch_b(orc)[2],):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_a_device(capi, orc, bad_prior=False):
    """Batch A from device memory in one call: the whole-batch kernels in both outer iterations.  bad_prior: scan A_BAD_PRIOR gets a
    non-finite device prior record (all others: no prior), so the first solve leaves it with status MSFL_BAD_ARG and the second
    association pass meets a scan whose status is not 0."""
    import torch
    C_, co, S_, so, gs = batch_a(orc)
    _, mc, ms = common.small_world()
    dev = torch.device("cuda", 0)
    h = capi.Handle(0)
    try:
        h.set_map(mc, ms)
        dC, dS, dP = torch.from_numpy(C_).to(dev), torch.from_numpy(S_).to(dev), torch.from_numpy(gs.copy()).to(dev)
        dSt = torch.full((A_SCANS,), 77, dtype=torch.int32, device=dev)
        if bad_prior:
            rec = capi.pose_priors(np.tile([0, 0, 0, 0, 0, 0, 1.0], (A_SCANS, 1)), np.zeros((A_SCANS, 6, 6)))
            rec["pose"][A_BAD_PRIOR, 1] = np.nan
            d_prior = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to(dev)
            h.set_pose_prior_device(d_prior, A_SCANS)
        torch.cuda.synchronize()
        info = (capi.MatchInfo * A_SCANS)()
        s = h.lib.msfl_match_scan2map_batch(h.h, C.c_int(A_SCANS), capi._vp(dC), capi._vp(co), capi._vp(dS), capi._vp(so), capi._vp(dP),
                                            capi._vp(dSt), info, C.c_int(capi.MEM_DEVICE))
        h._check(s, "msfl_match_scan2map_batch(device)")
        h.synchronize()
        return result(dP.cpu().numpy(), dSt.cpu().numpy(), info)
    finally:
        h.close()


def run_a_pinned(capi, orc, monkeypatch):
    """Batch A from pinned host buffers in two parts of A_PART_SCANS scans: each part's first association pass follows the copy
    through the per-record kernels, its second pass runs the whole-batch kernels over the same record buffer."""
    import torch
    C_, co, S_, so, gs = batch_a(orc)
    _, mc, ms = common.small_world()
    monkeypatch.setenv("MSFL_H2D_CHUNK_SCANS", str(A_PART_SCANS))
    h = capi.Handle(0)
    try:
        h.set_map(mc, ms)
        pC, pS = torch.from_numpy(C_).pin_memory(), torch.from_numpy(S_).pin_memory()
        poses, status, info = h.match_scan2map_batch(pC.numpy(), co, pS.numpy(), so, gs, want_info=True)
        return result(poses, status, info)
    finally:
        h.close()


def run_b(capi, orc, reject):
    """Batch B as one host batch and as three single calls (two dicts).  reject: threshold rejection in front of every solve."""
    cs, ss, gs = batch_b(orc)
    _, mc, ms = common.small_world()
    co = np.cumsum([0] + [len(c) for c in cs]).astype(np.int32)
    so = np.cumsum([0] + [len(s) for s in ss]).astype(np.int32)
    h = capi.Handle(0)
    try:
        h.set_map(mc, ms)
        if reject:
            h.set_outlier_rejection(threshold=B_REJECT_THRESHOLD, which=capi.REJECT_EVERY_OUTER, n=len(gs))
        poses, status, info = h.match_scan2map_batch(np.concatenate(cs), co, np.concatenate(ss), so, gs, want_info=True)
        batch = result(poses, status, info)
        if reject:
            batch["n_plane_rejected"] = h.rejection()["n_plane_rejected"].astype(np.int32)
        singles = [h.match_scan2map(cs[b], ss[b], gs[b]) for b in range(len(gs))]
        single = result([p for _, p, _ in singles], [s for s, _, _ in singles], [i for _, _, i in singles])
        return batch, single
    finally:
        h.close()


def all_runs(capi, orc, monkeypatch):
    """name -> result dict of every run the fixture holds."""
    out = {"a_device": run_a_device(capi, orc), "a_device_bad_prior": run_a_device(capi, orc, True), "a_pinned": run_a_pinned(capi, orc, monkeypatch)}
    for reject in (False, True):
        batch, single = run_b(capi, orc, reject)
        out["b_batch" + ("_reject" if reject else "")] = batch
        out["b_single" + ("_reject" if reject else "")] = single
    return out
