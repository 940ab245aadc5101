#!/usr/bin/env python3
"""Records tests/golden/lm_pipeline_parent_v1.npz: what the LM solve returned for every case of tests/lm_pipeline_cases.py in the
commit before round 7 (bbbc0ba: tr_decide / tr_propose as calls).  Needs a GPU.

    git worktree add /tmp/parent bbbc0ba  &&  make -C /tmp/parent/msf_loam_amd/csrc
    MSFL_LIB=/tmp/parent/msf_loam_amd/libmsfl_hip.so python tests/golden/make_lm_pipeline_golden.py

The fixture holds results only: poses, costs, counts.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from msf_loam_amd import capi
    from tests import lm_pipeline_cases as pc
    if not os.environ.get("MSFL_LIB"):
        raise SystemExit("set MSFL_LIB to the library of the commit before round 7 (see the docstring)")
    got = pc.solve_all(capi)
    names = np.array([c.name for c in pc.CASES])
    by = {c.name: i for i, c in enumerate(pc.CASES)}
    # what the special cases are for must hold in the recording itself
    assert got["lm_iterations"][by["at_minimum"]] == 0, "at_minimum: the first tr_propose must return 0"
    assert got["lm_iterations"][by["one_pass"]] == 1, "one_pass: exactly one later pass"
    i = by["all_rejected"]
    assert got["pose"][i].tobytes() == np.asarray(pc.problem(i).guess).tobytes(), "all_rejected: the pose passes through"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lm_pipeline_parent_v1.npz")
    np.savez_compressed(out, names=names, **got)
    print("wrote %s: %d cases, library %s" % (out, len(names), capi.LIB_PATH))


if __name__ == "__main__":
    main()
