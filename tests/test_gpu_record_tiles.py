"""Plane records in lane-transposed tiles of 64 rows, and the whole-batch 5-NN lists kept inside those tiles: a permutation of
where the same bits live, so every result equals, bit for bit, what the row-major layout gave.  The expected values were recorded
from the library of the commit before the tiles (tests/golden/make_record_tiles_golden.py -> tests/golden/record_tiles_parent_v1.npz);
the batches are described in tests/record_tiles_cases.py."""
import numpy as np
import pytest

from tests import record_tiles_cases as rt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(oracle):
    g = np.load(rt.GOLDEN)
    assert bytes(g["inputs_sha256"]).hex() == rt.inputs_digest(oracle), "the synthetic inputs are not the ones the fixture was recorded for"
    return g


def _same(golden, name, got):
    for k, v in got.items():
        want = golden[name + "/" + k]
        assert v.dtype == want.dtype and v.shape == want.shape, (name, k)
        assert np.array_equal(v, want), (name, k, np.argwhere(v != want)[:4].tolist())


def test_whole_batch_path_equals_the_row_major_layout(golden, oracle):
    """(a) 14 scans from device memory, >= 65 536 records: whole-batch kernels in both passes; scans start at 13 residue classes mod 64,
    partial last tile, non-zero first offsets, a scan without surf and one without corner features."""
    from msf_loam_amd import capi
    _, co, _, so, _ = rt.batch_a(oracle)
    assert co[0] == rt.A_C0 and so[0] == rt.A_S0 and (so[-1] - so[0]) % 64 != 0 and (co[-1] - co[0]) + (so[-1] - so[0]) >= 65536
    assert so[rt.A_NO_SURF + 1] == so[rt.A_NO_SURF] and co[rt.A_NO_CORNER + 1] == co[rt.A_NO_CORNER]
    got = rt.run_a_device(capi, oracle)
    assert not got["status"].any()
    _same(golden, "a_device", got)


def test_whole_batch_path_with_a_scan_that_failed_in_the_first_pass(golden, oracle):
    """(a) again, scan 6 with a non-finite prior record: its status is 3 when the second 5-NN pass runs, whose lanes of that scan
    write 'no neighbours' into the tiles; the other scans do not notice."""
    from msf_loam_amd import capi
    got = rt.run_a_device(capi, oracle, bad_prior=True)
    assert got["status"][rt.A_BAD_PRIOR] == 3 and np.count_nonzero(got["status"]) == 1
    _same(golden, "a_device_bad_prior", got)
    keep = np.arange(rt.A_SCANS) != rt.A_BAD_PRIOR
    assert np.array_equal(got["poses"][keep], golden["a_device/poses"][keep])


def test_pinned_host_batch_mixes_both_kernel_families_on_one_handle(golden, oracle, monkeypatch):
    """(c) batch (a) from pinned host buffers in two parts: per-record kernels behind the copies, then the whole-batch kernels over
    the same record buffer.  Equals the fixture and therefore (a)."""
    from msf_loam_amd import capi
    got = rt.run_a_pinned(capi, oracle, monkeypatch)
    _same(golden, "a_pinned", got)
    for k in rt.FIELDS:
        assert np.array_equal(golden["a_pinned/" + k], golden["a_device/" + k]), k


@pytest.mark.parametrize("reject", [False, True], ids=["plain", "threshold_rejection_every_outer"])
def test_per_record_path_on_a_tiny_batch(golden, oracle, reject):
    """(b) 3 scans with surf counts (130, 64, 61) and corner counts (0, 7, 70) as one batch and as three single calls; once more with
    threshold rejection in front of every solve, whose zeroed rows land mid-tile."""
    from msf_loam_amd import capi
    cs, ss, _ = rt.batch_b(oracle)
    assert tuple(len(s) for s in ss) == rt.B_SURF and tuple(len(c) for c in cs) == rt.B_CORNER
    batch, single = rt.run_b(capi, oracle, reject)
    tag = "_reject" if reject else ""
    _same(golden, "b_batch" + tag, batch)
    _same(golden, "b_single" + tag, single)
    for k in rt.FIELDS:
        assert np.array_equal(batch[k], single[k]), k
    if reject:
        assert (batch["n_plane_rejected"] > 0).any()
