#!/usr/bin/env python3
"""Records tests/golden/reg_options_parent_v1.npz: what the calls of tests/reg_options_cases.py returned in the commit before the
registration options and record sinks got one shape (83ceebf: four hand-rolled sink sets in the handle, four in the SLAM session).
Needs a GPU.

    git worktree add /tmp/parent 83ceebf  &&  make -C /tmp/parent/msf_loam_amd/csrc
    MSFL_LIB=/tmp/parent/msf_loam_amd/libmsfl_hip.so python tests/golden/make_reg_options_golden.py

Every case runs twice and the two runs must agree byte for byte before anything is written, so the fixture holds only what the parent
itself reproduces from run to run.  Nothing had to be left out: poses, statuses, counts, info records and all side records were stable.
The fixture holds results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("MSFL_LIB"):
        raise SystemExit("set MSFL_LIB to the library of the parent commit (see the docstring)")
    import torch
    torch.zeros(1, device="cuda:0")             # torch's HIP context goes first (tests/conftest.py)
    from msf_loam_amd import capi
    from oracle import oracle as orc
    from tests import reg_options_cases as rc
    from tests.test_gpu_rejection import _slam_scans
    orc.build()
    orc.lib()
    got, unstable = {}, []
    for case in rc.CASES:
        a = rc.run(capi, orc, _slam_scans(), case)
        b = rc.run(capi, orc, _slam_scans(), case)
        for key in a:
            if a[key].tobytes() != b[key].tobytes():
                unstable.append(key)
        got.update(a)
    assert not unstable, "not stable from run to run on this library: %s" % unstable
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "reg_options_parent_v1.npz")
    np.savez_compressed(out, **got)
    print("wrote %s: %d arrays, %d bytes, library %s" % (out, len(got), sum(v.nbytes for v in got.values()), capi.LIB_PATH))

    # what the session is for must hold in the recording itself (checked last, so that a recording that misses it can be looked at)
    for mode in ("sync", "pipelined"):
        st = {n: got["slam_%s_%s_status" % (mode, n)].tolist() for n in ("unc", "degen", "rej", "win")}
        assert st["unc"] == st["degen"] == [capi.BAD_ARG] * 2 + [capi.OK] * 4, st
        assert st["rej"] == [capi.BAD_ARG] * 2 + [capi.OK] * 3 + [capi.BAD_ARG] and st["win"] == [capi.OK] * 6, st
        win = got["slam_%s_win" % mode]
        assert [bool(w.any()) for w in win] == [False, False, False, True, False, True], "crops after scans 3 and 5 only"

if __name__ == "__main__":
    main()
