#!/usr/bin/env python3
"""Records tests/golden/graph_loss_parent_v1.npz: what msfl_graph_* returned for the runs of tests/graph_loss_parent_cases.py in the
commit before a loss per factor was added (224d569).  Needs a GPU.

    git worktree add /tmp/parent 224d569  &&  make -C /tmp/parent/msf_loam_amd/csrc
    MSFL_LIB=/tmp/parent/msf_loam_amd/libmsfl_hip.so python tests/golden/make_graph_loss_parent_golden.py

The parent's library has no msfl_graph_set_losses; the run calls nothing newer than msfl_graph_marginals.  The whole sequence runs twice
and the two runs must agree byte for byte before anything is written, so the fixture holds only what the parent itself reproduces from
run to run.
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
    from tests import graph_loss_parent_cases as pc
    a = pc.run(capi)
    b = pc.run(capi)
    unstable = [k for k in a if a[k].tobytes() != b[k].tobytes()]
    assert sorted(a) == sorted(b) and not unstable, "not stable from run to run on this library: %s" % unstable
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "graph_loss_parent_v1.npz")
    np.savez_compressed(out, **a)
    print("wrote %s: %d arrays, %d bytes, library %s" % (out, len(a), sum(v.nbytes for v in a.values()), capi.LIB_PATH))
    for name in pc.CASES:
        print(name, "summary", np.frombuffer(a["summary_" + name].tobytes(), np.int32)[:4].tolist(), "accepted", a["acc_" + name].tolist())


if __name__ == "__main__":
    main()
