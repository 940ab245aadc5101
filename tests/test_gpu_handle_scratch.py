"""GPU: the handle's named scratch sets (ExtractScratch, OdomScratch, VoxelScratch, PointPassScratch, DeskewScratch, PairScratch,
ScoreScratch in msfl_api.hip, the named buffers of msfl_places_s) hold what the numbered slot arrays before them held.
tests/golden/handle_scratch_parent_v1.npz was recorded from the parent commit's library (tests/golden/make_handle_scratch_golden.py:
every array there agreed between two runs of that library), the calls are those of tests/handle_scratch_cases.py (one handle through
every host-memory call three times over, small - large - small, then the voxel forms the sequence does not reach), and every
comparison here is of bytes: nothing the calls return is left out.
"""
import os

import numpy as np
import pytest

from tests import handle_scratch_cases as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handle_scratch_parent_v1.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
def test_one_handle_through_every_call_is_bit_identical_to_the_parent(gpu, golden):
    from msf_loam_amd import capi
    got = hc.run(capi)
    assert sorted(got) == sorted(golden) and len(golden) > 200
    wrong = []
    for key in sorted(golden):
        assert got[key].dtype == golden[key].dtype and got[key].shape == golden[key].shape, key
        if got[key].dtype == np.int32:
            print(key, got[key].tolist())
        if got[key].tobytes() != golden[key].tobytes():
            wrong.append(key)
    assert not wrong, wrong


def test_the_sequence_covers_what_it_is_for(golden):
    """(No GPU needed.)"""
    from msf_loam_amd import capi
    hc.check_coverage(golden, capi)
