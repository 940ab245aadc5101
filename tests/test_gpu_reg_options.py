"""GPU: the host plumbing of what a registration call carries (RegOptions, RecordSink, SlotRecords: msfl_api.hip, msfl_api_slam.inc)
computes what the hand-rolled copies before it did.  tests/golden/reg_options_parent_v1.npz was recorded from the parent commit's
library (tests/golden/make_reg_options_golden.py: every array there agreed between two runs of that library), the calls are those of
tests/reg_options_cases.py, and every comparison here is of bytes: poses, statuses, info records, the record sinks of the batch
matcher through host and device memory, the four side-record pairs of every scan of a SLAM session whose features are switched
mid-session, and which of their getters refuse.
"""
import os

import numpy as np
import pytest

from tests import reg_options_cases as rc
from tests.test_gpu_rejection import _slam_scans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reg_options_parent_v1.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.CASES)
def test_results_are_bit_identical_to_the_parent(gpu, oracle, golden, case):
    from msf_loam_amd import capi
    got = rc.run(capi, oracle, _slam_scans(), case)
    want = {k: v for k, v in golden.items() if k.startswith(case + "_")}
    assert sorted(got) == sorted(want) and len(want) >= 6
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if key.endswith("_status"):
            print(key, got[key].tolist())
        if got[key].ndim == 2:                          # per scan of the session: name the scan
            for k in range(len(want[key])):
                assert got[key][k].tobytes() == want[key][k].tobytes(), (key, "scan", k)
        assert got[key].tobytes() == want[key].tobytes(), key


def test_the_session_covers_every_transition(golden):
    """(No GPU needed.)  What the fixture is for: scans 0-1 fed with everything off (their getters refuse), a crop on every second scan from scan 2 on,
    rejection cleared for scan 5 while the other records go on, and the mapping prior of scan 3 moving that scan's mapping solve."""
    from msf_loam_amd import capi
    for mode in ("sync", "pipelined"):
        st = {n: golden["slam_%s_%s_status" % (mode, n)].tolist() for n in ("unc", "degen", "rej", "win")}
        assert st["unc"] == st["degen"] == [capi.BAD_ARG] * 2 + [capi.OK] * 4
        assert st["rej"] == [capi.BAD_ARG] * 2 + [capi.OK] * 3 + [capi.BAD_ARG]
        assert st["win"] == [capi.OK] * 6
        assert [bool(w.any()) for w in golden["slam_%s_win" % mode]] == [False, False, False, True, False, True]
        for name in ("unc", "degen", "rej"):
            assert [bool(r.any()) for r in golden["slam_%s_%s" % (mode, name)]][:2] == [False, False]
            assert golden["slam_%s_%s" % (mode, name)][4].any()                 # scan 4 reuses slot 0, which scan 0 left unarmed
    for key in ("rec", "unc", "degen", "rej", "win"):
        assert golden["slam_sync_" + key].tobytes() == golden["slam_pipelined_" + key].tobytes(), key
    for key in ("poses", "status", "info", "unc", "degen", "rej"):
        assert golden["batch_host_" + key].tobytes() == golden["batch_device_" + key].tobytes(), key
