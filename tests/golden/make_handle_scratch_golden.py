#!/usr/bin/env python3
"""Records tests/golden/handle_scratch_parent_v1.npz: what the calls of tests/handle_scratch_cases.py returned in the commit before
the handle's numbered scratch arrays (dk[5], ex[16], od[20], vb[14], vb2[6], pp[5], pr[5], sc[8], msfl_places_s::sp[]) became named
buffer sets (da2e8cd).  Needs a GPU.

    git worktree add /tmp/parent da2e8cd  &&  make -C /tmp/parent/msf_loam_amd/csrc
    MSFL_LIB=/tmp/parent/msf_loam_amd/libmsfl_hip.so python tests/golden/make_handle_scratch_golden.py

The whole sequence runs twice and the two runs must agree byte for byte before anything is written, so the fixture holds only what the
parent itself reproduces from run to run.  Nothing had to be left out.  The fixture holds results only: counts, statuses, poses and info
records in full, SHA-1 digests of every large array.
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
    from tests import handle_scratch_cases as hc
    a = hc.run(capi)
    b = hc.run(capi)
    unstable = [k for k in a if a[k].tobytes() != b[k].tobytes()]
    assert sorted(a) == sorted(b) and not unstable, "not stable from run to run on this library: %s" % unstable
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "handle_scratch_parent_v1.npz")
    np.savez_compressed(out, **a)
    print("wrote %s: %d arrays, %d bytes, library %s" % (out, len(a), sum(v.nbytes for v in a.values()), capi.LIB_PATH))
    for k in sorted(a):
        if a[k].dtype == np.int32:
            print(k, a[k].tolist())
    # what the sequence is for must hold in the recording itself (checked last, so that a recording that misses it can be looked at)
    hc.check_coverage(a, capi)


if __name__ == "__main__":
    main()
