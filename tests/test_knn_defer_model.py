"""The deferred 5-NN walk (knn5_grid_k32<.., DEFER>: capped row visits, the rest of a long range walked after the ninth row),
restated on the CPU in tests/knn_defer_model.py on top of tests/knn_grid_model.py.

  exact           for every case of tests/knn_grid_cases.py, every pose and every table cap of the grid model, the deferred order
                  returns the brute-force top five by (f32 distance, index) of every query whose 5th distance is inside the gate,
                  and its 5th distance is the one oracle.knn_brute finds: with the shipped caps and stack depth, and with caps of one
                  pair-iteration at stack depths 1 and 4, where nearly every visited row defers and the stack fills.
  not vacuous     over the cases, ranges were deferred and ranges were walked in place on a full stack, in each of the three settings.
"""
import functools

import numpy as np
import pytest

from tests import knn_defer_model as dm
from tests import knn_grid_cases as gc
from tests import knn_grid_model as gm
from tests.test_knn_grid_model import _pairs            # the brute-force top fives of the in-gate queries, computed once

GATE = np.float32(1.0)
ONES = (1,) * 9
SETTINGS = (("shipped", dm.SHIPPED_CAPS, dm.SHIPPED_DEPTH), ("ones, depth 1", ONES, 1), ("ones, depth 4", ONES, 4))
_seen = {s[0]: {"deferred": 0, "in_place": 0, "queries": 0} for s in SETTINGS}


def _descs(cloud):
    """The distinct descriptors the table caps give this cloud."""
    out = {}
    for cap in gm.CAPS:
        g = gm.desc_of(cloud, cap)
        out.setdefault((g.dims, float(g.inv), float(g.inv_x)), g)
    return list(out.values())


@functools.lru_cache(maxsize=None)
def _run(name):
    """Walks every in-gate query of the case under every descriptor and setting; returns the misses."""
    misses = []
    for kind, cloud, Q, P, D, qid in _pairs(name):
        first = np.flatnonzero(np.r_[True, qid[1:] != qid[:-1]])         # one row of five per query
        q, d4 = Q[first], D[first]
        for g in _descs(cloud):
            ix = dm.Index(cloud, g)
            su = dm.setup(ix, q)
            for i in range(len(q)):
                d2 = gm.l2_simple(ix.pts, q[i])
                want = dm.brute_top5(ix, d2, GATE)
                assert len(want) == 5 and np.float32(want[4][0]) == d4[i], (name, kind, i, want, d4[i])      # the oracle's 5th distance
                top, st = dm.walk(ix, su, i, d2, float(GATE))
                if top != want:
                    misses.append((name, kind, g.dims, "plain", q[i], top, want))
                for label, caps, depth in SETTINGS:
                    top, st = dm.walk(ix, su, i, d2, float(GATE), caps, depth)
                    if top != want:
                        misses.append((name, kind, g.dims, label, q[i], top, want))
                    seen = _seen[label]
                    seen["deferred"] += st["deferred"]; seen["in_place"] += st["in_place"]; seen["queries"] += 1
    return misses


@pytest.mark.parametrize("name", gc.NAMES)
def test_the_deferred_order_returns_the_brute_force_top_five(oracle, name):
    misses = _run(name)
    assert not misses, "%d misses, first: %s" % (len(misses), misses[0])


def test_deferral_and_the_full_stack_path_occurred(oracle):
    for name in ("generic", "lattice", "faces"):
        _run(name)
    print(_seen)
    for label, seen in _seen.items():
        assert seen["queries"] > 1000, (label, seen)
        assert seen["deferred"] > 0, (label, seen)
        assert seen["in_place"] > 0, (label, seen)
