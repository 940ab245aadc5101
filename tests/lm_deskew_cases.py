"""The case table of tests/test_gpu_lm_deskew.py (GPU) and tests/test_lm_deskew_cases_model.py (CPU): fixed-record problems for
msfl_solve_records_deskew whose row counts sit on the seams of the DE-SKEW branch of evaluate_pass<BLOCK, FILL>
(msf_loam_amd/csrc/msfl_kernels.cuh, pprime != nullptr): its own edge loop (`k += BLOCK` over the dense list of kEdgeListMax
entries plus the checked tail, no grouped loads) and the plain plane loop (`i += BLOCK`, no LDS cache), points read as f64 p'.

TEST INFRASTRUCTURE.  Every problem is the `_synthetic_corr` recipe of tests/test_gpu_scan2map.py (f32 points in +-20 m, random
unit normals, noise 0.01, a guess 0.2 m / 2 degrees off the truth) with a motion of its own per row:

    p'_i = dq_i p_i + dp_i      in f64, dq_i a rotation of up to 0.3 rad about a random axis, dp_i up to 0.2 m per axis

corr["p"] is p' (not representable in f32), C is generated from p', and the clouds staged with the call carry the ORIGINAL p_i as
f32.  A kernel that reads the cloud, or a cache of f32 points, instead of p' is off by decimetres.  Both references (the oracle's
solve and the numpy Jacobian) are computed once per case and shared; nobody writes to them.
"""
import collections
import functools

import numpy as np

from msf_loam_amd import synth
from tests import lm_boundary_cases as lb

BLOCKS = lb.BLOCKS
CACHE = lb.CACHE                     # the plain branch's LDS plane cache: the de-skew branch must not use it
EDGE_LIST_MAX = lb.EDGE_LIST_MAX
GROUP = {128: 8, 512: 4}             # kGroup = lm_load_group(BLOCK): the plain branch's grouped plane loads, not taken here either
MAX_ANGLE, MAX_SHIFT = 0.3, 0.2      # per-row motion: rad, metres per axis

PATTERNS = ("edge_bit0", "edge_bit31", "edge_tail_only", "edge_head_only", "plane_last_rejected", "all_rejected", "empty")


def edge_counts(block):
    """With 300 planes: one mask word +-1; BLOCK +-1; kEdgeListMax +-1; the tail; the count of the `many_edges` case."""
    return [1, 31, 32, 33, block - 1, block, block + 1, 1023, 1024, 1025, 1536, 2600]


def plane_counts(block):
    """With 40 edges below 200 planes and none from 200 up: 1; BLOCK +-1; CACHE +-1; one whole grouped trip of the plain branch past it."""
    cache = CACHE[block]
    return [1, block - 1, block, block + 1, cache - 1, cache, cache + 1, cache + GROUP[block] * block + 1]


Case = collections.namedtuple("Case", "k block ns nc pattern")


def _pattern_sizes(block, pattern):
    if pattern.startswith("edge_"):
        return 300, 2600
    if pattern.startswith("plane_"):
        return CACHE[block] + 200, 0
    return (300, 40) if pattern == "all_rejected" else (0, 0)


def _table():
    out = []
    for block in BLOCKS:
        for nc in edge_counts(block):
            out.append((block, 300, nc, "none"))
        for ns in plane_counts(block):
            out.append((block, ns, 40 if ns < 200 else 0, "none"))
        for pattern in PATTERNS:
            out.append((block,) + _pattern_sizes(block, pattern) + (pattern,))
    return [Case(k, *c) for k, c in enumerate(out)]


CASES = _table()
# the sibling kernels (prior, rejection, degeneracy), one problem per width: past the plain branch's cache and past the edge list
SIBLINGS = {block: Case(len(CASES) + j, block, CACHE[block] + 200, 1100, "none") for j, block in enumerate(BLOCKS)}
_ALL = CASES + [SIBLINGS[b] for b in BLOCKS]


def case_id(c):
    return "k%d-b%d-ns%d-nc%d-%s" % (c.k, c.block, c.ns, c.nc, c.pattern)


is_void = lb.is_void
rejected_rows = lb.rejected_rows     # (the patterns shared with the plain table reject the same rows)


def seam_rows(c):
    """Record indices at the seams of case c, accepted or not: rows BLOCK - 1 / BLOCK of either loop, around the edge list, around
    the plain branch's cache, the last edge and the last row."""
    cache = CACHE[c.block]
    rows = [c.nc + i for i in (c.block - 1, c.block, cache - 1, cache) if 0 <= i < c.ns]
    rows += [i for i in (c.block - 1, c.block, EDGE_LIST_MAX - 1, EDGE_LIST_MAX) if i < c.nc]
    if c.nc + c.ns:
        rows.append(c.nc + c.ns - 1)
        if c.nc and c.ns:
            rows.append(c.nc - 1)
    return sorted(set(rows))


def deskew_corr(rng, n_plane, n_edge, noise):
    """`_synthetic_corr` with a motion per row -> (corr with p = p', truth, the original f32 points p as f64)."""
    from oracle.oracle import CORR
    n = n_edge + n_plane
    truth = np.array([0.3, -0.2, 0.1, 0, 0, np.sin(0.05), np.cos(0.05)])
    R = synth.quat_to_matrix(truth[3:])
    corr = np.zeros(n, dtype=CORR)
    p = rng.uniform(-20, 20, (n, 3)).astype(np.float32).astype(np.float64)          # features are f32 points
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(-MAX_ANGLE, MAX_ANGLE, n)
    dp = rng.uniform(-MAX_SHIFT, MAX_SHIFT, (n, 3))
    # Rodrigues, row by row: p' = p cos a + (k x p) sin a + k (k.p) (1 - cos a) + dp
    ca, sa = np.cos(angle)[:, None], np.sin(angle)[:, None]
    pp = p * ca + np.cross(axis, p) * sa + axis * (axis * p).sum(1, keepdims=True) * (1 - ca) + dp
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    slide = np.where(np.arange(n) < n_edge, rng.normal(size=n), 0.0)[:, None]     # an edge point slides along N
    corr["p"], corr["N"] = pp, N
    corr["kind"] = np.where(np.arange(n) < n_edge, 1, 2)
    corr["C"] = pp @ R.T + truth[:3] + noise * rng.normal(size=(n, 3)) + N * slide
    return corr, truth, p


Problem = collections.namedtuple("Problem", "case corr truth guess corner surf rec points accepted")


@functools.lru_cache(maxsize=None)
def problem(k):
    """The problem of case k: correspondences (p = p') for the references; clouds (the ORIGINAL f32 points), records and points for
    msfl_solve_records_deskew."""
    c = _ALL[k]
    rng = np.random.default_rng(4100 + k)
    corr, truth, p = deskew_corr(rng, n_plane=c.ns, n_edge=c.nc, noise=0.01)
    guess = synth.perturb_pose(truth, rng, 0.2, 2.0)
    drop = rejected_rows(c)
    corr["kind"][drop] = 0
    corr["N"][drop] = 0.0
    corr["C"][drop] = 0.0
    corner = np.concatenate([p[:c.nc], np.zeros((c.nc, 1))], 1).astype(np.float32)
    surf = np.concatenate([p[c.nc:], np.zeros((c.ns, 1))], 1).astype(np.float32)
    rec = np.concatenate([corr["C"], corr["N"]], 1)
    points = np.array(corr["p"])
    for a in (corr, truth, guess, corner, surf, rec, points):
        a.setflags(write=False)
    return Problem(c, corr, truth, guess, corner, surf, rec, points, np.flatnonzero(corr["kind"] != 0))


def with_cloud_points(p):
    """The correspondences of problem p with f32(p) -- what the staged clouds hold -- in place of p': the model of a kernel that
    reads the cloud instead of the points."""
    corr = np.array(p.corr)
    corr["p"] = np.concatenate([p.corner[:, :3], p.surf[:, :3]]).astype(np.float64)
    return corr


@functools.lru_cache(maxsize=None)
def oracle_solution(k):
    """(pose, summary) of oracle.ceres_solve on problem k from its guess."""
    from oracle import oracle as orc
    orc.build()
    p = problem(k)
    return orc.ceres_solve(np.array(p.corr), np.array(p.guess))
