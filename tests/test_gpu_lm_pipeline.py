"""GPU: the LM solve across its pass boundaries, bit for bit against the commit before round 7 (docs/kernels/scan2map.md).

Round 7 inlined tr_decide / tr_propose into lm_solve_kernel<128> and measured (and dropped) requesting the next pass's first streamed
rows under the reduction and lane 0's step.  Neither may change a result: every thread takes its rows in ascending order, a pass sums
{cached planes, edges, streamed planes}, and the trust-region step is the same arithmetic.  tests/golden/lm_pipeline_parent_v1.npz was
recorded from the parent commit's library (tests/golden/make_lm_pipeline_golden.py), and every comparison here is np.array_equal.

Cases (tests/lm_pipeline_cases.py), all on the default 128-thread workgroup through Handle.solve_records:
  boundary-*   the width-128 non-void cases of tests/lm_boundary_cases.py (prior cases through lm_solve_prior_kernel)
  shape-*      832 + {1, 63, 64, 65, 127, 128, 129, 1 023, 1 024, 1 025, 2 053} plane rows x {0, 3, 1 030} corner rows: the first
               streamed group of a later pass empty, partial across the two wavefronts, exactly full, one past full
  head_all / head_alternate   rejected rows (N = 0) over that whole group / every other row of it
  at_minimum   the first tr_propose returns 0; all_rejected: nothing to solve (msfl_solve_records asks for no minimum number of
               correspondences, so the status is 0 and the pose passes through); one_pass: the solve ends after one later pass
and one batch of three bench-world scans through match_scan2map_batch against the three single-scan calls.
"""
import os

import numpy as np
import pytest

from tests import lm_pipeline_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_pipeline_parent_v1.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert [str(n) for n in g["names"]] == [c.name for c in pc.CASES], "fixture and case table differ: re-record the fixture"
    return g


@pytest.fixture(scope="module")
def solved(gpu):
    from msf_loam_amd import capi
    return pc.solve_all(capi)


@pytest.mark.parametrize("i", range(len(pc.CASES)), ids=[c.name for c in pc.CASES])
def test_solve_is_bit_identical_to_the_parent(solved, golden, i):
    c = pc.CASES[i]
    print("%s: ns %d nc %d  iterations %d successful %d  cost %.17g -> %.17g  (parent %d %d %.17g -> %.17g)"
          % (c.name, c.ns, c.nc, solved["lm_iterations"][i], solved["lm_successful"][i], solved["initial_cost"][i], solved["final_cost"][i],
             golden["lm_iterations"][i], golden["lm_successful"][i], golden["initial_cost"][i], golden["final_cost"][i]))
    for f in pc.FIELDS:
        assert np.array_equal(solved[f][i], golden[f][i]), (c.name, f, solved[f][i], golden[f][i])
    assert solved["pose"][i].tobytes() == golden["pose"][i].tobytes()


def test_solves_that_end_early(solved, golden):
    """The three early ends, as the recording has them: no later pass, nothing to solve (the pose's bytes are the guess's), one
    later pass."""
    by = {c.name: i for i, c in enumerate(pc.CASES)}
    assert solved["lm_iterations"][by["at_minimum"]] == 0 and golden["lm_iterations"][by["at_minimum"]] == 0
    i = by["all_rejected"]
    assert solved["pose"][i].tobytes() == np.asarray(pc.problem(i).guess).tobytes()
    assert solved["status"][i] == golden["status"][i] and solved["lm_iterations"][i] == 0
    assert solved["lm_iterations"][by["one_pass"]] == 1 and golden["lm_iterations"][by["one_pass"]] == 1


def test_batch_of_three_equals_three_single_calls(gpu):
    """Bench-world features with surf counts on either side of cache + one group (832 + 1 024 rows): the batch launch and the
    single-scan launches run the same solve kernel on the same rows, so poses and info records agree bit for bit."""
    from msf_loam_amd import capi, synth
    world = synth.World(ground_half=synth.ground_half_for_target(30000))
    mc, ms = synth.make_map(world)
    truths = synth.random_poses(3, synth.SEED + 77)
    rng = np.random.default_rng(77)
    corner, surf, guesses = [], [], []
    for b, want in enumerate((pc.CACHE + 1024 - 37, pc.CACHE + 1024, pc.CACHE + 1024 + 301)):
        pts, ring, kind = synth.make_scan(world, truths[b], synth.SEED + 78 + b, with_kind=True)
        c, s = synth.direct_features(pts, kind)
        assert len(s) >= want, (len(s), want)
        corner.append(c); surf.append(s[:want]); guesses.append(synth.perturb_pose(truths[b], rng))
    co = np.cumsum([0] + [len(c) for c in corner]).astype(np.int32)
    so = np.cumsum([0] + [len(s) for s in surf]).astype(np.int32)
    h = capi.Handle(0)
    try:
        h.set_map(mc, ms)
        poses, status, info = h.match_scan2map_batch(np.concatenate(corner), co, np.concatenate(surf), so, np.stack(guesses), want_info=True)
        for b in range(3):
            s1, p1, i1 = h.match_scan2map(corner[b], surf[b], guesses[b])
            print("scan %d: surf %d corner %d  planes %s  iterations %s" % (b, len(surf[b]), len(corner[b]), list(i1.n_plane), list(i1.lm_iterations)))
            assert s1 == status[b] == 0
            assert np.asarray(p1, np.float64).tobytes() == poses[b].tobytes(), b
            for f, _ in capi.MatchInfo._fields_:
                a, g = getattr(i1, f), getattr(info[b], f)
                assert (a == g) if f == "status" else (list(a) == list(g)), (b, f)
            assert i1.n_plane[0] > pc.CACHE                      # rows are streamed at all
    finally:
        h.close()
