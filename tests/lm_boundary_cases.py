"""The case table of tests/test_gpu_lm_boundaries.py (GPU) and tests/test_lm_boundary_cases_model.py (CPU): fixed-record
problems whose row counts sit on the structural seams of evaluate_pass<BLOCK, FILL> (msf_loam_amd/csrc/msfl_kernels.cuh).

TEST INFRASTRUCTURE.  Every problem is the `_synthetic_corr` recipe of tests/test_gpu_scan2map.py (f32 points in +-20 m,
random unit normals) with noise 0.01 and a guess 0.2 m / 2 degrees off the truth, seeded from the case's index in CASES.
Both references (the oracle's solve and the numpy Jacobian) are computed once per case and shared; nobody writes to them.
"""
import collections
import functools

import numpy as np

from msf_loam_amd import synth
from tests.test_gpu_scan2map import _synthetic_corr

# ---- the constants the sizes come from (msfl_kernels.cuh / msfl_api_slam.inc) ----
BLOCKS = (128, 512)                  # kLmBlock, kSlamLmBlock
CACHE = {128: 832, 512: 3072}        # lm_plane_cache(BLOCK): plane rows kept in LDS
EDGE_LIST_MAX = 1024                 # kEdgeListMax: edges with an index below it go through the 32 x 32-bit mask and the dense list
# kGroup = lm_load_group(BLOCK) = 8 / 4: the streamed plane loop loads kGroup * BLOCK rows per trip (clamped index);
# kEdgeGroup = 4 / 1: the edge walk loads kEdgeGroup * BLOCK rows per trip

# plane counts (with 40 edges while ns < 200, else none)
PLANE_COUNTS = {
    # 1; BLOCK +-1; cache +-1; 7 x BLOCK +-1 (832 = 6.5 x 128: lanes 0..63 cache seven rows, the others six); cache + kGroup * BLOCK +-1
    # (one whole streamed trip); 15 x BLOCK; cache + 2 x kGroup x BLOCK + 1
    128: [1, 127, 128, 129, 831, 832, 833, 895, 896, 897, 1855, 1856, 1857, 1920, 2881],
    # 1; BLOCK +-1; cache +-1; cache + BLOCK +-1; cache + kGroup * BLOCK +-1; past it
    512: [1, 511, 512, 513, 3071, 3072, 3073, 3583, 3584, 3585, 5119, 5120, 5121, 6000],
}
# edge counts (with 300 planes)
EDGE_COUNTS = {
    # one mask word +-1; BLOCK +-1; kEdgeGroup * BLOCK +-1; kEdgeListMax +-1; the tail; the count of the `many_edges` case
    128: [1, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1536, 2600],
    512: [1, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 1536, 2600],
}
# rejected-record patterns (kind 0, N = C = 0), each at both widths; sizes in _pattern_sizes
PATTERNS = ("edge_bit0", "edge_bit31", "edge_tail_only", "edge_head_only", "plane_seam_rejected", "plane_seam_only",
            "plane_last_rejected", "all_rejected", "empty")
PRIOR_SEED = 7000                    # the prior of case k is drawn from default_rng(PRIOR_SEED + k)

Case = collections.namedtuple("Case", "k block ns nc pattern prior")


def _pattern_sizes(block, pattern):
    """(ns, nc) of a pattern: edge patterns need rows on both sides of kEdgeListMax, plane patterns on both sides of the cache."""
    if pattern.startswith("edge_"):
        return 300, 2600
    if pattern.startswith("plane_"):
        return CACHE[block] + 200, 0
    return (300, 40) if pattern == "all_rejected" else (0, 0)


def _table():
    out = []
    for block in BLOCKS:
        for ns in PLANE_COUNTS[block]:
            out.append((block, ns, 40 if ns < 200 else 0, "none", False))
        for nc in EDGE_COUNTS[block]:
            out.append((block, 300, nc, "none", False))
        for pattern in PATTERNS:
            out.append((block,) + _pattern_sizes(block, pattern) + (pattern, False))
    for block in BLOCKS:                                     # lm_solve_prior_kernel is a kernel text of its own
        out += [(block, CACHE[block] - 1, 0, "none", True), (block, CACHE[block] + 1, 0, "none", True), (block, 300, 1025, "none", True)]
    return [Case(k, *c) for k, c in enumerate(out)]


CASES = _table()
WIDTH_PAIR = Case(len(CASES), 0, 3500, 1100, "none", False)     # one problem solved at both widths (block 0: the caller picks)


def case_id(c):
    return "k%d-b%d-ns%d-nc%d-%s%s" % (c.k, c.block, c.ns, c.nc, c.pattern, "-prior" if c.prior else "")


def is_void(c):
    """No accepted row: the solve must leave the pose alone."""
    return c.pattern in ("all_rejected", "empty")


def rejected_rows(c):
    """Indices into the record list [edges | planes] that the pattern rejects."""
    e, p = np.arange(c.nc), c.nc + np.arange(c.ns)
    cache = CACHE.get(c.block, 0)
    seam = c.nc + np.arange(cache - 2, cache + 2)
    if c.pattern == "edge_bit0":
        return e[e % 32 != 0]
    if c.pattern == "edge_bit31":
        return e[e % 32 != 31]
    if c.pattern == "edge_tail_only":
        return e[:EDGE_LIST_MAX]
    if c.pattern == "edge_head_only":
        return e[EDGE_LIST_MAX:]
    if c.pattern == "plane_seam_rejected":
        return seam
    if c.pattern == "plane_seam_only":                       # of the 64 rows around the seam only the four at it stay
        return np.setdiff1d(c.nc + np.arange(cache - 32, cache + 32), seam)
    if c.pattern == "plane_last_rejected":
        return p[-1:]
    if c.pattern == "all_rejected":
        return np.concatenate([e, p])
    return np.zeros(0, np.int64)


Problem = collections.namedtuple("Problem", "case corr truth guess corner surf rec accepted")


@functools.lru_cache(maxsize=None)
def problem(k):
    """The problem of case k (k = len(CASES): WIDTH_PAIR): correspondences for the references, arrays for msfl_solve_records."""
    c = CASES[k] if k < len(CASES) else WIDTH_PAIR
    rng = np.random.default_rng(100 + k)
    corr, truth = _synthetic_corr(rng, n_plane=c.ns, n_edge=c.nc, noise=0.01)
    guess = synth.perturb_pose(truth, rng, 0.2, 2.0)
    drop = rejected_rows(c)
    corr["kind"][drop] = 0
    corr["N"][drop] = 0.0
    corr["C"][drop] = 0.0
    corner = np.concatenate([corr["p"][:c.nc], np.zeros((c.nc, 1))], 1).astype(np.float32)
    surf = np.concatenate([corr["p"][c.nc:], np.zeros((c.ns, 1))], 1).astype(np.float32)
    rec = np.concatenate([corr["C"], corr["N"]], 1)
    for a in (corr, truth, guess, corner, surf, rec):
        a.setflags(write=False)
    return Problem(c, corr, truth, guess, corner, surf, rec, np.flatnonzero(corr["kind"] != 0))


@functools.lru_cache(maxsize=None)
def oracle_solution(k):
    """(pose, summary) of oracle.ceres_solve on problem k from its guess."""
    from oracle import oracle as orc
    orc.build()
    p = problem(k)
    return orc.ceres_solve(np.array(p.corr), np.array(p.guess))


def prior_of(k):
    """(mean pose, sqrt information) of a prior case: full rank, mean a few centimetres off the truth."""
    from tests import prior_numpy as pn
    rng = np.random.default_rng(PRIOR_SEED + k)
    mean = synth.perturb_pose(np.array(problem(k).truth), rng, max_t=0.05, max_deg=0.5)
    return mean, pn.random_spd_sqrt(rng)


def seam_rows(c):
    """Record indices at the seams of case c, accepted or not: around the plane cache, around the edge list, the last row."""
    cache = CACHE.get(c.block, 0)
    rows = [c.nc + i for i in (cache - 1, cache) if 0 <= i < c.ns]
    rows += [i for i in (EDGE_LIST_MAX - 1, EDGE_LIST_MAX) if i < c.nc]
    if c.nc + c.ns:
        rows.append(c.nc + c.ns - 1)
        if c.nc and c.ns:
            rows.append(c.nc - 1)                            # the last edge row as well
    return sorted(set(rows))
