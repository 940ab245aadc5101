"""GPU: the scan-to-map 5-NN index at its geometric limits -- cell size, bounding-box faces, degenerate boxes, long thin boxes and
the life of the shared count table across builds.  The cases are tests/knn_grid_cases.py; the geometry itself (which cells the
walk may skip) is pinned on the CPU by tests/test_knn_grid_model.py.

An exact top five by (distance, index) does not depend on the cell size, the walk's form or the build path, so:

  cap sweep       MSFL_GRID_CAP_CELLS in {8, 64, 4 096, default} x MSFL_KNN_FORM in {lane, rows}: msfl_associate_scan2map records
                  bit-identical across the eight handles on every case; accept sets equal to oracle.associate_scan2map(...,
                  use_kdtree=False) and accepted records within 1e-9 of it (docs/parity.md; line directions free in sign);
                  msfl_match_scan2map on the generic case bit-identical across handles
  coarse grid     knn_candidates (msfl_set_timing(h, 3)) at cap 8 and 64 strictly above the default's, with equal records; and
                  at caps 8, 64 and 4 096 no more than the model allows for a walk that prunes at the gate (bounds in metres)
  per-kind kernel the generic and lattice jobs tiled to >= 65 536 features in one batch at cap 64 against single calls at the default
  build paths     MSFL_INDEX_SINGLE=1 against the pair build, at cap 64 and at the default, the empty and tiny maps included
  pairs           msfl_match_pairs_batch on (generic, rod_x_2.7km) against single calls
  table life      the sequence knn_grid_cases.TABLE_LIFE of msfl_set_map calls on ONE handle (spans grow and shrink, the pair
                  and single build paths alternate, a one-point map in between): after every call the records equal those of a
                  fresh handle given only that map; with the default cap and with MSFL_GRID_CAP_CELLS=65536, and each of the
                  two again with MSFL_INDEX_SINGLE=1 on the long-lived handle
  non-finite      the generic map with NaN / Inf points interleaved gives the oracle's records on the map without them

A map of fewer than five points is refused (MSFL_MAP_TOO_SMALL) by every handle alike; the build has run by then.
The environment is read when a handle is created; every handle of a test lives in this one process.
"""
import functools

import numpy as np
import pytest

from tests import knn_grid_cases as gc
from tests import knn_grid_model as gm

pytestmark = pytest.mark.gpu

CAPS = (8, 64, 4096, None)            # None: the default (1 M cells on a handle's first build, then what the map wanted)
FORMS = ("lane", "rows")
TOO_SMALL = "MAP_TOO_SMALL"


def _handle(cap=None, form=None, single=False):
    from msf_loam_amd import capi
    with pytest.MonkeyPatch.context() as mp:
        for name, value in (("MSFL_GRID_CAP_CELLS", cap), ("MSFL_KNN_FORM", form), ("MSFL_INDEX_SINGLE", 1 if single else None)):
            if value is None:
                mp.delenv(name, raising=False)
            else:
                mp.setenv(name, str(value))
        return capi.Handle(0)


@pytest.fixture(scope="module")
def handles(gpu):
    hs = {(cap, form): _handle(cap, form) for cap in CAPS for form in FORMS}
    yield hs
    for h in hs.values():
        h.close()


def _associate(h, c, pose):
    """Records, or TOO_SMALL when the handle refuses the map."""
    from msf_loam_amd import capi
    try:
        return h.associate_scan2map(c.corner, c.surf, pose)
    except capi.MsflError as e:
        assert e.status == capi.MAP_TOO_SMALL, e
        return TOO_SMALL


def _first_diff(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return None if (isinstance(a, str) and isinstance(b, str) and a == b) else -1
    rows = np.flatnonzero((a != b).any(1))
    return int(rows[0]) if len(rows) else None


def _assert_same(a, b, what):
    k = _first_diff(a, b)
    if k is not None:
        detail = "one side refused the map" if k < 0 else "first differing query %d: %s vs %s" % (k, a[k], b[k])
        raise AssertionError("%s: %s" % (what, detail))


@functools.lru_cache(maxsize=None)
def _oracle_corr(name, k):
    from oracle import oracle as orc
    orc.build()
    c = gc.case(name)
    return orc.associate_scan2map(c.mc, c.ms, c.corner, c.surf, c.poses[k], use_kdtree=False)


def _check_against_oracle(rec, corr, nc, what):
    ok_o = corr["kind"] != 0
    ok_g = np.any(rec[:, 3:] != 0, axis=1)
    if not np.array_equal(ok_g, ok_o):
        k = int(np.flatnonzero(ok_g != ok_o)[0])
        raise AssertionError("%s: accept sets differ, first at query %d (GPU %s, oracle %s)" % (what, k, ok_g[k], ok_o[k]))
    pl = ok_o.copy(); pl[:nc] = False
    ed = ok_o.copy(); ed[nc:] = False
    err = np.zeros(len(rec))
    if pl.any():
        err[pl] = np.maximum(np.abs(rec[pl, :3] - corr["C"][pl]).max(1), np.abs(rec[pl, 3:] - corr["N"][pl]).max(1))
    if ed.any():
        n_dot = np.abs(np.sum(rec[ed, 3:] * corr["N"][ed], axis=1))                  # eigenvector sign is free
        d = rec[ed, :3] - corr["C"][ed]                                              # C = centre +- 0.1 dir: distance from the centre line
        perp = d - np.sum(d * corr["N"][ed], axis=1, keepdims=True) * corr["N"][ed]
        err[ed] = np.maximum(np.abs(n_dot - 1), np.abs(perp).max(1))
    bad = np.flatnonzero(err >= 1e-9)
    assert len(bad) == 0, "%s: record of query %d is %.3e from the oracle's (%s vs C %s N %s)" % (
        what, bad[0], err[bad[0]], rec[bad[0]], corr["C"][bad[0]], corr["N"][bad[0]])
    return int(ed.sum()), int(pl.sum()), float(err.max()) if len(err) else 0.0


# accepted (edges, planes) every case must at least give at its first pose, so that "equal" is not "equally empty"
MIN_ACCEPTED = {"generic": (60, 80), "lattice": (20, 500), "faces": (60, 300), "flat_z": (25, 100), "line_corner": (50, 15),
                "corner_5pt": (15, 15), "corner_5same": (0, 15), "surf_5pt": (30, 15), "gate_reach": (5, 900)}


@pytest.mark.parametrize("name", gc.NAMES)
def test_records_do_not_depend_on_the_cell_size_or_the_walk(handles, oracle, name):
    c = gc.case(name)
    for h in handles.values():
        h.set_map(c.mc, c.ms)
    grown = {cap: (gm.desc_of(c.mc, cap or gm.DEFAULT_CAP).steps, gm.desc_of(c.ms, cap or gm.DEFAULT_CAP).steps) for cap in CAPS}
    for k, pose in enumerate(c.poses):
        recs = {key: _associate(h, c, pose) for key, h in handles.items()}
        first = recs[(None, "rows")]
        for (cap, form), rec in recs.items():
            _assert_same(rec, first, "case %s pose %d: cap %s form %s against the default cap, rows form" % (name, k, cap, form))
        if gc.too_small(c):
            assert first == TOO_SMALL, "case %s: a map of fewer than five points was accepted" % name
            continue
        n_e, n_p, err = _check_against_oracle(first, _oracle_corr(name, k), len(c.corner), "case %s pose %d" % (name, k))
        print("%-14s pose %d: edges %d planes %d accepted, largest record error %.3e; cell-edge growth steps (corner, surf) per cap %s"
              % (name, k, n_e, n_p, err, grown))
        want = MIN_ACCEPTED.get(name, (30, 150))           # the rods: 36 edges and 180 planes asked for
        if k == 0:
            assert n_e >= want[0] and n_p >= want[1], (name, n_e, n_p)
    for cloud in (c.mc, c.ms):                             # the smallest cap really grows the edge
        if len(cloud):
            g8 = gm.desc_of(cloud, 8)
            assert g8.steps > 0 or g8.want_cells <= 8, (name, g8)


def test_registration_does_not_depend_on_the_cell_size_or_the_walk(handles):
    c = gc.case("generic")
    for h in handles.values():
        h.set_map(c.mc, c.ms)
    for k, pose in enumerate(c.poses):
        out = {key: h.match_scan2map(c.corner, c.surf, pose) for key, h in handles.items()}
        s0, p0, i0 = out[(None, "rows")]
        assert s0 == 0 and i0.n_plane[0] >= 80 and i0.n_edge[0] >= 60 and i0.lm_iterations[0] > 0
        for (cap, form), (s, p, info) in out.items():
            what = "generic pose %d cap %s form %s" % (k, cap, form)
            assert s == s0 and np.array_equal(p, p0), "%s: pose %s vs %s" % (what, p, p0)
            for f in ("n_edge", "n_plane", "lm_iterations", "final_cost"):
                assert list(getattr(info, f)) == list(getattr(i0, f)), "%s: %s %s vs %s" % (what, f, list(getattr(info, f)), list(getattr(i0, f)))


@pytest.mark.parametrize("name", ["generic", "rod_y_12km"])
def test_the_coarse_grid_was_really_used(handles, name):
    c = gc.case(name)
    counts, recs = {}, {}
    for cap in (8, 64, None):
        h = handles[(cap, "lane")]
        h.set_map(c.mc, c.ms)
        h.set_timing(3)
        try:
            h.get_timing(reset=True)
            recs[cap] = h.associate_scan2map(c.corner, c.surf, c.poses[0])
            counts[cap] = h.get_timing(reset=True).knn_candidates
        finally:
            h.set_timing(0)
    print("%s: candidates evaluated per cap %s" % (name, counts))
    for cap in (8, 64):
        _assert_same(recs[cap], recs[None], "case %s, counting 5-NN, cap %s against the default" % (name, cap))
        assert counts[cap] > counts[None] > 0, (name, counts)
    assert counts[8] >= counts[64]
    handles[(None, "rows")].set_map(c.mc, c.ms)
    _assert_same(recs[None], handles[(None, "rows")].associate_scan2map(c.corner, c.surf, c.poses[0]), "case %s, counting 5-NN against the rows form" % name)


@pytest.mark.parametrize("cap", [8, 64, 4096])
def test_a_coarse_grid_still_prunes_by_metres(handles, cap):
    """The lower bounds are distances: cells away times the cell edge the descriptor really has.  At d4 = the gate the model
    gives the most candidates any visit order can evaluate (knn_grid_model.candidates_upper_bound); a walk that measured a
    grown grid with the base edge would stay exact and visit nearly the whole neighbourhood instead."""
    c = gc.case("generic")
    bound = full = 0
    for cloud, q in ((c.mc, c.corner), (c.ms, c.surf)):
        b, f = gm.candidates_upper_bound(gm.desc_of(cloud, cap), cloud, q[:, :3], np.float32(1.0))      # poses[0] is the identity
        bound, full = bound + b, full + f
    h = handles[(cap, "lane")]
    h.set_map(c.mc, c.ms)
    h.set_timing(3)
    try:
        h.get_timing(reset=True)
        h.associate_scan2map(c.corner, c.surf, c.poses[0])
        n = h.get_timing(reset=True).knn_candidates
    finally:
        h.set_timing(0)
    print("generic, cap %d: %d candidates evaluated; the model allows %d, the whole neighbourhood holds %d" % (cap, n, bound, full))
    assert 0 < n <= bound, (cap, n, bound)
    if cap >= 64:
        assert 2 * bound < full            # not vacuous: the bound is far below the neighbourhood


@pytest.mark.parametrize("name", ["generic", "lattice"])
def test_per_kind_kernel_on_a_coarse_grid(handles, name):
    c = gc.case(name)
    n_feat = len(c.corner) + len(c.surf)
    B = -(-65536 // n_feat)
    co, so = np.arange(B + 1, dtype=np.int32) * len(c.corner), np.arange(B + 1, dtype=np.int32) * len(c.surf)
    assert co[-1] + so[-1] >= 65536
    guesses = np.array([c.poses[i % len(c.poses)] for i in range(B)])
    coarse, ref = handles[(64, "lane")], handles[(None, "rows")]
    coarse.set_map(c.mc, c.ms)
    ref.set_map(c.mc, c.ms)
    pb, sb, ib = coarse.match_scan2map_batch(np.tile(c.corner, (B, 1)), co, np.tile(c.surf, (B, 1)), so, guesses, want_info=True)
    for i, pose in enumerate(c.poses):
        s1, p1, i1 = ref.match_scan2map(c.corner, c.surf, pose)
        assert i1.n_plane[0] > 50
        for j in range(i, B, len(c.poses)):
            what = "case %s, batch entry %d (cap 64, per-kind kernel) against a single call at the default cap" % (name, j)
            assert sb[j] == s1 and np.array_equal(pb[j], p1), "%s: pose %s vs %s" % (what, pb[j], p1)
            for f in ("n_edge", "n_plane", "lm_iterations", "final_cost"):
                assert list(getattr(ib[j], f)) == list(getattr(i1, f)), "%s: %s" % (what, f)


def test_single_and_pair_builds_agree_on_coarse_and_default_grids():
    hs = {(cap, single): _handle(cap, None, single) for cap in (64, None) for single in (False, True)}
    try:
        # empty and tiny maps between full ones: the pair chain serves two non-empty clouds, the single builds everything else
        order = ("generic", "empty_corner", "faces", "empty_surf", "corner_1pt", "corner_5pt", "flat_z", "corner_4pt", "rod_x_6km",
                 "surf_5pt", "line_corner", "generic")
        for step, name in enumerate(order):
            c = gc.case(name)
            for h in hs.values():
                h.set_map(c.mc, c.ms)
            for k, pose in enumerate(c.poses):
                recs = {key: _associate(h, c, pose) for key, h in hs.items()}
                for (cap, single), rec in recs.items():
                    _assert_same(rec, recs[(None, False)], "step %d case %s pose %d: cap %s %s build against the default cap, pair build"
                                 % (step, name, k, cap, "single" if single else "pair"))
                assert isinstance(recs[(None, False)], str) == gc.too_small(c), name
    finally:
        for h in hs.values():
            h.close()


def test_pairs_batch_equals_single_calls_on_a_rod(gpu):
    names = ("generic", "rod_x_2.7km")
    cs = [gc.case(n) for n in names]
    off = lambda arrs: np.cumsum([0] + [len(a) for a in arrs]).astype(np.int32)
    guesses = np.array([cs[0].poses[1], cs[1].poses[1]])
    poses, status, info = gpu.match_pairs_batch(np.concatenate([c.mc for c in cs]), off([c.mc for c in cs]),
                                                np.concatenate([c.ms for c in cs]), off([c.ms for c in cs]),
                                                np.concatenate([c.corner for c in cs]), off([c.corner for c in cs]),
                                                np.concatenate([c.surf for c in cs]), off([c.surf for c in cs]), guesses, want_info=True)
    h = _handle()
    try:
        for p, c in enumerate(cs):
            h.set_map(c.mc, c.ms)
            s1, p1, i1 = h.match_scan2map(c.corner, c.surf, guesses[p])
            what = "pair %d (%s) of msfl_match_pairs_batch against msfl_match_scan2map" % (p, names[p])
            assert status[p] == s1 == 0 and np.array_equal(poses[p], p1), "%s: status %d / %d, pose %s vs %s" % (what, status[p], s1, poses[p], p1)
            assert i1.n_plane[0] >= 80 and i1.n_edge[0] >= 30
            for f in ("n_edge", "n_plane", "lm_iterations", "final_cost"):
                assert list(getattr(info[p], f)) == list(getattr(i1, f)), "%s: %s" % (what, f)
    finally:
        h.close()


@pytest.mark.parametrize("cap,single", [(None, False), (65536, False), (None, True), (65536, True)],
                         ids=["default", "cap65536", "default-single", "cap65536-single"])
def test_table_life_across_builds_of_one_handle(cap, single):
    """Spans grow (rod_y_12km wants 384 k cells at the base edge) and shrink back, the pair and the single build paths alternate,
    and a one-point map is built in between: the shared count table must come back all zero from every build.  single: the
    long-lived handle builds every map with MSFL_INDEX_SINGLE=1, so the single build's report of the wanted table size is what
    sets every later span."""
    def records(h, c):
        return [_associate(h, c, pose) for pose in c.poses]

    fresh = {}
    for name in sorted(set(gc.TABLE_LIFE)):
        h = _handle(cap)
        try:
            c = gc.case(name)
            h.set_map(c.mc, c.ms)
            fresh[name] = records(h, c)
        finally:
            h.close()
    assert fresh["corner_1pt"][0] == TOO_SMALL and fresh["empty_corner"][0] == TOO_SMALL and not isinstance(fresh["generic"][0], str)
    h = _handle(cap, single=single)
    try:
        for step, name in enumerate(gc.TABLE_LIFE):
            c = gc.case(name)
            h.set_map(c.mc, c.ms)
            for k, (a, b) in enumerate(zip(records(h, c), fresh[name])):
                _assert_same(a, b, "cap %s%s, step %d (%s), pose %d: the long-lived handle against a fresh one"
                             % (cap or "default", ", single builds" if single else "", step, name, k))
    finally:
        h.close()


def test_non_finite_map_points_are_skipped(handles, oracle):
    c = gc.case("generic")
    rng = np.random.default_rng(77)
    mc, ms = gc.with_non_finite(rng, c.mc, 7), gc.with_non_finite(rng, c.ms, 5)
    assert len(ms) == len(c.ms) + len(c.ms) // 5 and not np.isfinite(ms[:, :3]).all()
    for (cap, form) in ((64, "lane"), (None, "lane"), (None, "rows")):
        h = handles[(cap, form)]
        h.set_map(mc, ms)
        for k, pose in enumerate(c.poses):
            rec = h.associate_scan2map(c.corner, c.surf, pose)
            n_e, n_p, _ = _check_against_oracle(rec, _oracle_corr("generic", k), len(c.corner), "generic map with NaN / Inf points, cap %s form %s pose %d" % (cap, form, k))
            assert n_e >= 60 and n_p >= 80
