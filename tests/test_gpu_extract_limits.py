"""GPU: stage A (feature extraction) at its structural limits, on every form of the ring split.

The cases are tests/extract_limit_cases.py's; tests/test_extract_limit_cases_model.py proves on the CPU that each one sits where its
name claims.  Five handles, MSFL_PREP_SPLIT = 1, 2, 4, 8 and 16: G = 1 is the one-workgroup prepare kernel that every large batch runs
and that the default handle never reaches below 129 scans; the others are the three-launch form, and the compact kernel's piece loop
follows the same G.  Every case runs on all five, once alone and once inside a batch between two other cases.

  across the five G   every output array is identical as bytes (times included) and the status is equal
  against the oracle  status, rings, xyz, curvature bits, labels and the four lists are exact; the relative time is within
                      np.spacing(float32(0.2)), the bound tests/test_gpu_extract.py uses for device atan2 against libm, and its "more
                      than 99 % of the times bit-equal" holds over the pooled points of all cases (one differing ulp in a cloud of 63
                      points is 1.6 % of that cloud)
  a refused scan      has no features (and no points, unless it is MSFL_CAPACITY, which keeps the ring-split cloud it could not
                      pick from); its good neighbours in the batch equal their single-call results bit for bit
"""
import os

import numpy as np
import pytest

from tests import extract_limit_cases as ec

pytestmark = pytest.mark.gpu

ARRAYS = ("full", "ring", "curvature", "label", "sharp", "less_sharp", "flat", "less_flat")
TIME_BOUND = np.spacing(np.float32(0.2))


@pytest.fixture(scope="module")
def handles():
    """One handle per G, and the default one (G by batch size)."""
    from msf_loam_amd import capi
    saved = os.environ.pop("MSFL_PREP_SPLIT", None)
    hs = {}
    try:
        hs["default"] = capi.Handle(0)
        for G in ec.SPLITS:
            os.environ["MSFL_PREP_SPLIT"] = str(G)
            hs[G] = capi.Handle(0)
        del os.environ["MSFL_PREP_SPLIT"]
        yield hs
    finally:
        os.environ.pop("MSFL_PREP_SPLIT", None)
        for h in hs.values():
            h.close()
        if saved is not None:
            os.environ["MSFL_PREP_SPLIT"] = saved


_REFS = {}


def _reference(cloud):
    """The oracle's result for a cloud of the table, computed once (keyed by the cloud's identity: the table caches its cases)."""
    from oracle import oracle as orc
    key = id(cloud[0])
    if key not in _REFS:
        orc.build()
        _REFS[key] = (cloud, orc.extract_features(cloud[0], cloud[1]))
    return _REFS[key][1]


def _extract(h, clouds):
    off = np.cumsum([0] + [len(p) for p, _ in clouds]).astype(np.int32)
    pts = np.concatenate([p for p, _ in clouds]) if off[-1] else np.zeros((0, 4), np.float32)
    ring = np.concatenate([r for _, r in clouds]) if off[-1] else np.zeros(0, np.uint16)
    return h.extract_features_batch(pts, ring, off)


def _same_bytes(f, g):
    return f["rc"] == g["rc"] and all(f[k].shape == g[k].shape and np.array_equal(f[k].view(np.uint8), g[k].view(np.uint8)) for k in ARRAYS)


def _check_refused(tag, f, status):
    assert f["rc"] == status, (tag, f["rc"], status)
    for k in ("sharp", "less_sharp", "flat", "less_flat"):
        assert len(f[k]) == 0, (tag, k)
    if status != ec.CAPACITY:
        assert len(f["full"]) == 0, tag


def _check_oracle(tag, f, fo):
    """Everything but the time exact, the time within the bound; returns (times that differ in bits, times)."""
    assert f["rc"] == fo["rc"] == 0, (tag, f["rc"], fo["rc"])
    assert np.array_equal(f["ring"], fo["ring"]), tag
    assert np.array_equal(f["full"][:, :3].view(np.uint32), fo["full"][:, :3].view(np.uint32)), tag
    assert np.array_equal(f["curvature"].view(np.uint32), fo["curvature"].view(np.uint32)), tag
    assert np.array_equal(f["label"], fo["label"]), (tag, np.flatnonzero(f["label"] != fo["label"])[:8])
    for k in ("sharp", "less_sharp", "flat", "less_flat"):
        assert np.array_equal(f[k], fo[k]), (tag, k, f[k][:8], fo[k][:8])
    dt = np.abs(f["full"][:, 3].astype(np.float64) - fo["full"][:, 3].astype(np.float64))
    assert len(dt) == 0 or dt.max() <= TIME_BOUND, (tag, dt.max(), int(dt.argmax()))
    return int(np.sum(f["full"][:, 3].view(np.uint32) != fo["full"][:, 3].view(np.uint32))), len(dt)


_RESULTS = {}


def _run_case(handles, name):
    """The case on the five G, alone and inside a batch: checked, and its G = 1 results kept for the pooled share of equal times."""
    if name in _RESULTS:
        return _RESULTS[name]
    c = ec.case(name)
    front, back = (ec.case(n).clouds[0] for n in ec.SANDWICH)
    k = len(c.clouds)
    alone = {G: _extract(handles[G], c.clouds) for G in ec.SPLITS}
    inside = {G: _extract(handles[G], [front] + c.clouds + [back]) for G in ec.SPLITS}
    for G in ec.SPLITS:
        assert len(alone[G]) == k and len(inside[G]) == k + 2
        for b in range(k):                                       # across the five G, alone and inside: the same bytes
            assert _same_bytes(alone[G][b], alone[1][b]), (name, "alone", G, b)
            assert _same_bytes(inside[G][1 + b], alone[1][b]), (name, "inside", G, b)
        for b, cloud in ((0, front), (k + 1, back)):             # a case does not disturb its neighbours, refused or not
            assert _same_bytes(inside[G][b], inside[1][b]), (name, "neighbour", G, b)
    diff = total = 0
    for b, (cloud, status) in enumerate(zip(c.clouds, c.status)):
        if status != ec.OK:
            _check_refused((name, b), alone[1][b], status)
            continue
        d, t = _check_oracle((name, b), alone[1][b], _reference(cloud))
        diff += d; total += t
    for b, cloud in ((0, front), (k + 1, back)):
        _check_oracle((name, "neighbour", b), inside[1][b], _reference(cloud))
    _RESULTS[name] = (diff, total)
    return _RESULTS[name]


@pytest.mark.parametrize("name", ec.NAMES)
def test_case_on_every_ring_split_form(handles, name):
    diff, total = _run_case(handles, name)
    print("%-26s %7d points, %d times differ from the oracle's by one ulp" % (name, total, diff))


def test_relative_times_are_bit_equal_for_more_than_99_percent_of_all_points(handles):
    diff = total = 0
    for name in ec.NAMES:
        d, t = _run_case(handles, name)
        diff += d; total += t
    print("%d of %d times differ in bits" % (diff, total))
    assert total > 400000 and diff < 0.01 * total, (diff, total)


def test_refused_scans_between_good_ones(handles):
    """[good, empty, all-NaN, bad ring, 8 129-point ring, good] on the default handle and on every G: the statuses, nothing delivered
    for a refused scan, and the good scans equal their single-call results bit for bit (and the oracle)."""
    c = ec.case(ec.REFUSED_BATCH)
    for key, h in handles.items():
        res = _extract(h, c.clouds)
        assert [f["rc"] for f in res] == c.status, (key, [f["rc"] for f in res])
        for b, (cloud, status) in enumerate(zip(c.clouds, c.status)):
            if status != ec.OK:
                _check_refused((key, b), res[b], status)
                continue
            single = h.extract_features(cloud[0], cloud[1])
            assert all(np.array_equal(single[k].view(np.uint8), res[b][k].view(np.uint8)) for k in ARRAYS), (key, b)
            _check_oracle((key, b), res[b], _reference(cloud))
        assert len(res[4]["full"]) == ec.RING_CAPACITY + 1        # MSFL_CAPACITY keeps the cloud it could not pick from
        assert _same_bytes(res[0], _extract(h, c.clouds[:1])[0])      # the handle's next call is right


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_batch_sizes_on_either_side_of_every_threshold_of_g(handles, order):
    """B = 16 | 17, 32 | 33, 64 | 65, 128 | 129 tiny scans on ONE default handle: G = 16, 8, 4, 2 and the one-workgroup kernel in turn, the
    split scratch re-reserved in between.  Every scan equals the oracle, and its result on the forced G = 1 handle as bytes."""
    h = handles["default"]
    for B in (ec.B_EDGES if order == "ascending" else ec.B_EDGES[::-1]):
        clouds = ec.batch_of(B)
        res, res1 = _extract(h, clouds), _extract(handles[1], clouds)
        assert len(res) == B
        for b, cloud in enumerate(clouds):
            assert _same_bytes(res[b], res1[b]), (B, b)
            _check_oracle((B, b), res[b], _reference(cloud))
