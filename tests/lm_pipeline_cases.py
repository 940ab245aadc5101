"""The case table of tests/test_gpu_lm_pipeline.py and tests/golden/make_lm_pipeline_golden.py: fixed-record problems around the pass
boundary of the LM solve (msf_loam_amd/csrc/msfl_lm_solve_body.inc: last streamed row -> block_reduce -> lane 0's trust-region step ->
first row of the next pass; docs/kernels/scan2map.md, round 7).

TEST INFRASTRUCTURE.  The expected results are not computed here: they are what the library of the commit BEFORE round 7 returned for
these problems (tests/golden/lm_pipeline_parent_v1.npz), and the solve must reproduce them bit for bit -- round 7 changed how the
serial section is compiled (tr_decide / tr_propose inlined) and tried moving WHEN streamed rows are requested; neither may change
the order rows are summed in or what the trust-region step decides.  Problems are the `_synthetic_corr` recipe of
tests/test_gpu_scan2map.py, seeded per case; all on the default 128-thread solve workgroup through Handle.solve_records.
"""
import collections
import functools

import numpy as np

from msf_loam_amd import synth
from tests import lm_boundary_cases as lb
from tests.test_gpu_scan2map import _synthetic_corr

BLOCK = 128
CACHE = lb.CACHE[BLOCK]              # 832 rows stay in LDS; the streamed loop starts behind them
GROUP = 8                            # kGroup: trips per load group of the streamed loop; one group = GROUP * BLOCK rows
# rows behind the cache: first group of a later pass empty, partial across the two wavefronts (832 = 6.5 x 128: lanes 0..63 start one trip later),
# exactly one trip, one past it, one whole group +-1, and two groups and five rows
STREAMED = (1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2053)
CORNERS = (0, 3, 1030)               # no edge rows, fewer than one wavefront, past kEdgeListMax

# kind: how the problem is made and solved
#   boundary   problem k of tests/lm_boundary_cases.py (width 128, not void), with its prior where it has one
#   shape      ns = CACHE + streamed rows, nc corner rows
#   head_all / head_alternate   rows CACHE .. CACHE + GROUP * BLOCK - 1 rejected (N = C = 0): all of them / every other one
#   at_minimum     noise-free, guess = truth: the first tr_propose returns 0, no later pass runs
#   all_rejected   every row rejected: nothing to solve, the pose passes through
#   one_pass       max_lm_iterations = 1: the solve ends after exactly one later pass
Case = collections.namedtuple("Case", "name kind ns nc k")


def _table():
    out = []
    for c in lb.CASES:
        if c.block == BLOCK and not lb.is_void(c):
            out.append(Case("boundary-" + lb.case_id(c), "boundary", c.ns, c.nc, c.k))
    for nc in CORNERS:
        for s in STREAMED:
            out.append(Case("shape-ns%d-nc%d" % (CACHE + s, nc), "shape", CACHE + s, nc, None))
    out.append(Case("head_all", "head_all", CACHE + 2053, 3, None))
    out.append(Case("head_alternate", "head_alternate", CACHE + 2053, 3, None))
    out.append(Case("at_minimum", "at_minimum", 2000, 0, None))
    out.append(Case("all_rejected", "all_rejected", 2000, 40, None))
    out.append(Case("one_pass", "one_pass", 2000, 40, None))
    return out


CASES = _table()
Problem = collections.namedtuple("Problem", "case corner surf rec guess prior max_lm_iterations")


@functools.lru_cache(maxsize=None)
def problem(i):
    """Arrays for Handle.solve_records of CASES[i] (read-only, shared)."""
    c = CASES[i]
    if c.kind == "boundary":
        p = lb.problem(c.k)
        return Problem(c, p.corner, p.surf, p.rec, p.guess, lb.prior_of(c.k) if p.case.prior else None, None)
    rng = np.random.default_rng(9000 + i)
    corr, truth = _synthetic_corr(rng, n_plane=c.ns, n_edge=c.nc, noise=0.0 if c.kind == "at_minimum" else 0.01)
    guess = np.array(truth) if c.kind == "at_minimum" else synth.perturb_pose(truth, rng, 0.2, 2.0)
    head = c.nc + CACHE + np.arange(GROUP * BLOCK)
    drop = {"head_all": head, "head_alternate": head[::2], "all_rejected": np.arange(c.nc + c.ns)}.get(c.kind, np.zeros(0, np.int64))
    corr["N"][drop] = 0.0
    corr["C"][drop] = 0.0
    corner = np.concatenate([corr["p"][:c.nc], np.zeros((c.nc, 1))], 1).astype(np.float32)
    surf = np.concatenate([corr["p"][c.nc:], np.zeros((c.ns, 1))], 1).astype(np.float32)
    rec = np.concatenate([corr["C"], corr["N"]], 1)
    for a in (guess, corner, surf, rec):
        a.setflags(write=False)
    return Problem(c, corner, surf, rec, guess, None, 1 if c.kind == "one_pass" else None)


FIELDS = ("pose", "status", "initial_cost", "final_cost", "lm_iterations", "lm_successful")


def solve_all(capi):
    """Every case through Handle.solve_records on the loaded library -> {field: array with one row per case}.  Two handles: the
    default parameters, and max_lm_iterations = 1 for `one_pass`."""
    prm1 = capi.default_params()
    prm1.max_lm_iterations = 1
    handles = {None: capi.Handle(0), 1: capi.Handle(0, prm1)}
    out = {f: [] for f in FIELDS}
    try:
        for i in range(len(CASES)):
            p = problem(i)
            h = handles[p.max_lm_iterations]
            if p.prior is not None:
                h.set_pose_prior([p.prior[0]], [p.prior[1]])
            try:
                pose, info = h.solve_records(p.corner, p.surf, p.rec, p.guess)
            finally:
                if p.prior is not None:
                    h.clear_pose_prior()
            out["pose"].append(np.array(pose, np.float64))
            out["status"].append(info.status)
            for f in FIELDS[2:]:
                out[f].append(getattr(info, f)[0])
    finally:
        for h in handles.values():
            h.close()
    return {"pose": np.stack(out["pose"]), "status": np.array(out["status"], np.int32),
            "initial_cost": np.array(out["initial_cost"], np.float64), "final_cost": np.array(out["final_cost"], np.float64),
            "lm_iterations": np.array(out["lm_iterations"], np.int32), "lm_successful": np.array(out["lm_successful"], np.int32)}
