"""Writes tests/golden/record_tiles_parent_v1.npz: the runs of tests/record_tiles_cases.py through the library of the commit BEFORE
the record tiles (row-major plane records, 5-NN lists in a buffer of their own).  Build that commit's library and run, on the GPU,

    MSFL_LIB=/path/to/parent/libmsfl_hip.so python tests/golden/make_record_tiles_golden.py

The fixture holds, per run: poses, initial and final costs as f64 bit patterns, status, per-iteration correspondence counts and LM
iteration counts (and the per-scan rejected plane counts of the rejection runs), plus the sha256 of the inputs it belongs to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


class _Env:
    """monkeypatch.setenv for a script"""
    def setenv(self, k, v):
        os.environ[k] = v


def main():
    import torch
    torch.zeros(1, device="cuda:0")                  # torch's HIP context first (tests/conftest.py)
    from msf_loam_amd import capi
    from oracle import oracle as orc
    from tests import record_tiles_cases as rt
    orc.build(); orc.lib()
    assert os.environ.get("MSFL_LIB"), "point MSFL_LIB at the parent commit's library"
    runs = rt.all_runs(capi, orc, _Env())
    rej = runs["b_batch_reject"]["n_plane_rejected"]
    assert (rej > 0).any(), "the rejection threshold rejects no plane: the zeroing store is not exercised"
    a = runs["a_device_bad_prior"]
    assert a["status"][rt.A_BAD_PRIOR] == 3 and np.count_nonzero(a["status"]) == 1
    out = {name + "/" + k: v for name, r in runs.items() for k, v in r.items()}
    out["inputs_sha256"] = np.frombuffer(bytes.fromhex(rt.inputs_digest(orc)), np.uint8)
    np.savez_compressed(rt.GOLDEN, **out)
    print("wrote", rt.GOLDEN, os.path.getsize(rt.GOLDEN), "bytes;", "planes rejected per scan and iteration:", rej.tolist())


if __name__ == "__main__":
    main()
