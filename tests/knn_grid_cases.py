"""The case table of tests/test_knn_grid_model.py (CPU) and tests/test_gpu_knn_grid.py (GPU): maps and queries at the geometric
limits of the scan-to-map 5-NN index (msf_loam_amd/csrc/msfl_knn_index.cuh: grid_desc_from_bbox, grid_coord, axis_gap).

TEST INFRASTRUCTURE.  Seeded and deterministic; every case is (name, map_corner, map_surf, corner queries, surf queries,
poses), all clouds (n, 4) f32, poses (tx, ty, tz, qx, qy, qz, qw).  Cases are built once and shared; nobody writes to them.

  generic       3 000 surf points uniform in a 24 x 18 x 6 m box at (-7.3, 41.9, 2.2), 400 corner points on 8 segments; queries
                are jittered map points and uniform draws from the box inflated by 3 m.  No lattice: swapping one of the five
                neighbours moves the fitted record by far more than 1e-9, so the records pin the neighbour set.
  lattice       `_lattice_job` of tests/test_gpu_scan2map.py: ties, duplicates, the gate.
  faces         points exactly on the six faces, twelve edges and eight corners of the bounding box; queries on each face, one
                f32 step inside and outside it, at the radius outside +- one step, and 1, 2, 3, 3.5 and 4 cell edges outside
                (grid_coord's -2 and dim + 1 clamps), and round the corners.
  flat_z, line_corner, corner_1pt, corner_4pt, corner_5pt, corner_5same, surf_5pt, empty_corner, empty_surf
                degenerate boxes (an extent of 0 gives dims = 2) and tiny or empty maps.  A map of fewer than five points is
                refused by every registration entry point (MSFL_MAP_TOO_SMALL): `too_small(case)` says so, and what the GPU
                tests pin there is that the build itself leaves the handle sound.
  rod_x_0.9km, rod_x_2.7km, rod_x_6km, rod_y_2km, rod_y_8km, rod_y_12km
                three clusters of 300 surf points (two planes tilted 45 degrees against the rod) and 80 corner points, 2 m across, at the two ends and at 43 % of a long thin box.  A
                third of the surf points and of the queries are snapped, along the rod's axis, to f32 values within two steps of
                a COMPUTED cell boundary (half of them on the base-edge grid, half on the grid the descriptor really takes).
                All six fit the default 1 M-cell span at the base edge (43 k to 400 k cells); the ones with more than
                kGridMaxDim = 4 096 cells along the rod (x 2.7 km, x 6 km, y 8 km, y 12 km) get grown cells for that reason.
  gate_reach    330 probes per axis: a query whose only neighbours are five map points 0.995 m away along that axis (d^2 = 0.990 to
                0.991, inside the gate), the probes' positions stepping through every phase of the cell grid in 3.1 mm steps.  With
                the 0.1 % edge margin each group lies in the adjacent cell (x: within three sub-cells) at some phases by a hair;
                a cell edge below the radius puts it out of reach at those phases, at the base edge only.
  TABLE_LIFE    the sequence of msfl_set_map calls of the table-life test (one handle).
"""
import collections
import functools

import numpy as np

from tests import knn_grid_model as gm

F = np.float32
Case = collections.namedtuple("Case", "name mc ms corner surf poses")

IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])
SHIFT = np.array([0.05, -0.03, 0.02, 0, 0, 0, 1.0])
_q = np.array([0.004, -0.003, 0.006, 1.0]); _q /= np.linalg.norm(_q)
GENERIC_POSE = np.r_[0.21, -0.13, 0.08, _q]

RODS = {"rod_x_0.9km": (0, 900.0), "rod_x_2.7km": (0, 2700.0), "rod_x_6km": (0, 6000.0),
        "rod_y_2km": (1, 2000.0), "rod_y_8km": (1, 8000.0), "rod_y_12km": (1, 12000.0)}
DEGENERATE = ("flat_z", "line_corner", "corner_1pt", "corner_4pt", "corner_5pt", "corner_5same", "surf_5pt", "empty_corner", "empty_surf")
NAMES = ("generic", "lattice", "faces") + DEGENERATE + tuple(RODS) + ("gate_reach",)
TABLE_LIFE = ("generic", "rod_y_12km", "generic", "empty_corner", "generic", "corner_1pt", "lattice")


def pts4(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([xyz, np.zeros((len(xyz), 1), F)], 1), dtype=F)


def too_small(case):
    return min(len(case.mc), len(case.ms)) < 5


def _segments(rng, lo, ext, n_seg, n_per, jitter):
    out = []
    for _ in range(n_seg):
        a, b = lo + rng.uniform(0, 1, 3) * ext, lo + rng.uniform(0, 1, 3) * ext
        t = rng.uniform(0, 1, (n_per, 1))
        out.append(a + t * (b - a) + rng.normal(0, jitter, (n_per, 3)))
    return np.concatenate(out)


def _generic(rng):
    lo, ext = np.array([-7.3, 41.9, 2.2]), np.array([24.0, 18.0, 6.0])
    surf_map = lo + rng.uniform(0, 1, (3000, 3)) * ext
    corner_map = _segments(rng, lo, ext, 8, 50, 0.01)

    def queries(m, n_near, n_far):
        near = m[rng.integers(0, len(m), n_near)] + rng.normal(0, 0.15, (n_near, 3))
        far = (lo - 3.0) + rng.uniform(0, 1, (n_far, 3)) * (ext + 6.0)
        return np.concatenate([near, far])
    return Case("generic", pts4(corner_map), pts4(surf_map), pts4(queries(corner_map, 90, 30)), pts4(queries(surf_map, 450, 150)),
                (IDENTITY, GENERIC_POSE))


def _lattice(rng):
    from tests.test_gpu_scan2map import _lattice_job
    pole, lat, corner, surf = _lattice_job(np.random.default_rng(41))
    return Case("lattice", pole, lat, corner, surf, (IDENTITY, np.array([0.125, -0.25, 0.0, 0, 0, 0, 1.0])))


def _step(v, sign):
    return np.nextafter(F(v), F(np.inf) if sign > 0 else F(-np.inf))


def _faces(rng):
    lo = np.array([-3.7, 12.3, -1.1], F)
    hi = (lo + np.array([9.0, 7.0, 4.0], F)).astype(F)
    box = [lo, hi]
    ext = (hi - lo).astype(np.float64)
    inner = (lo + rng.uniform(0, 1, (1200, 3)) * ext).astype(F)
    surf_map, queries = [np.clip(inner, lo, hi)], []
    edge = gm.EDGE_MARGIN
    for a in range(3):
        others = [b for b in range(3) if b != a]
        for side in (0, 1):
            f, s = box[side][a], (1 if side else -1)
            on = (lo + rng.uniform(0, 1, (40, 3)) * ext).astype(F); on[:, a] = f
            surf_map.append(on)
            for _ in range(8):
                base = (lo + (0.1 + 0.8 * rng.uniform(0, 1, 3)) * ext).astype(F); base[a] = f
                near = np.repeat(base[None], 6, 0)
                near[:, others] += rng.uniform(-0.04, 0.04, (6, 2)).astype(F)
                surf_map.append(near)
                vals = [f, _step(f, s), _step(f, -s)]
                out_r = F(f + F(s))                                               # at the radius outside the face
                vals += [out_r, _step(out_r, s), _step(out_r, -s), F(f + F(s * 0.9)), F(f + F(s * 0.5)), F(f - F(s * 0.3))]
                ks = (1, 2, 3, 3.5, 4)
                vals += [F(f + F(s * k * edge)) for k in ks]
                if a == 0:
                    vals += [F(f + F(s * k * edge / gm.XSUB)) for k in ks + (7, 10)]
                for v in vals:
                    qq = base.copy(); qq[a] = v
                    queries.append(qq)
    corners = np.array([[box[i][0], box[j][1], box[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], F)
    signs = np.array([[2 * i - 1, 2 * j - 1, 2 * k - 1] for i in (0, 1) for j in (0, 1) for k in (0, 1)], F)
    surf_map.append(corners)
    round_corners = []
    for c, s in zip(corners, signs):
        round_corners += [c, np.array([_step(c[a], s[a]) for a in range(3)], F), np.array([_step(c[a], -s[a]) for a in range(3)], F)]
        for t in (0.3, 3.0 ** -0.5, 0.57, 0.58, 1.001, 2.1, 3.1, -0.2):
            round_corners.append((c + s * F(t)).astype(F))
    # the corner map: the twelve edges of the box (two coordinates exactly on a face)
    edges = []
    for a in range(3):
        others = [b for b in range(3) if b != a]
        for i in (0, 1):
            for j in (0, 1):
                e = np.zeros((30, 3), F)
                e[:, a] = (lo[a] + rng.uniform(0, 1, 30) * ext[a]).astype(F)
                e[:, others[0]], e[:, others[1]] = box[i][others[0]], box[j][others[1]]
                edges.append(e)
    edges = np.concatenate(edges + [corners])
    surf_q = np.concatenate([np.array(queries, F), np.array(round_corners, F)])
    corner_q = np.concatenate([(edges[rng.integers(0, len(edges), 60)] + rng.normal(0, 0.1, (60, 3))).astype(F), np.array(round_corners, F)])
    return Case("faces", pts4(edges), pts4(np.concatenate(surf_map)), pts4(corner_q), pts4(surf_q), (IDENTITY, SHIFT))


def _degenerate(name, rng):
    g = case("generic")
    if name == "flat_z":                    # extent 0 in z: dims[2] = 2
        lo = np.array([3.1, -8.2])
        xy = lo + rng.uniform(0, 1, (400, 2)) * np.array([8.0, 6.0])
        ms = np.concatenate([xy, np.full((400, 1), 1.5)], 1)
        seg = _segments(rng, np.r_[lo, 1.5], np.array([8.0, 6.0, 0.0]), 3, 40, 0.0); seg[:, 2] = 1.5
        surf = ms[rng.integers(0, 400, 120)] + rng.normal(0, 0.15, (120, 3)); surf[:40, 2] = 1.5
        corner = seg[rng.integers(0, len(seg), 30)] + rng.normal(0, 0.1, (30, 3)); corner[:10, 2] = 1.5
        return Case(name, pts4(seg), pts4(ms), pts4(corner), pts4(surf), (IDENTITY, SHIFT))
    if name == "line_corner":               # two extents 0 in the corner map
        x = np.sort(rng.uniform(-4.0, 15.0, 200))
        mc = np.stack([x, np.full(200, 47.25), np.full(200, 3.5)], 1)
        corner = mc[rng.integers(0, 200, 60)] + rng.normal(0, 0.2, (60, 3)); corner[:20, 1:] = (47.25, 3.5)
        return Case(name, pts4(mc), g.ms, pts4(corner), g.surf[:100], (IDENTITY, SHIFT))
    if name in ("corner_1pt", "corner_4pt", "corner_5pt", "corner_5same"):
        n = {"corner_1pt": 1, "corner_4pt": 4}.get(name, 5)
        mc = np.array([1.3, 50.2, 4.1]) + np.arange(n)[:, None] * np.array([0.11, 0.02, -0.03])
        if name == "corner_5same":
            mc = np.repeat(mc[:1], 5, 0)
        corner = mc[rng.integers(0, n, 24)] + rng.normal(0, 0.3, (24, 3))
        return Case(name, pts4(mc), g.ms, pts4(corner), g.surf[:100], (IDENTITY, SHIFT))
    if name == "surf_5pt":
        ms = np.array([[0.0, 0.0, 0.0], [0.31, 0.02, 0.0], [0.05, 0.27, 0.0], [0.36, 0.33, 0.0], [0.18, 0.15, 0.0]]) + np.array([2.0, 48.0, 5.0])
        surf = ms[rng.integers(0, 5, 24)] + rng.normal(0, 0.3, (24, 3))
        return Case(name, g.mc, pts4(ms), g.corner[:40], pts4(surf), (IDENTITY, SHIFT))
    if name == "empty_corner":
        return Case(name, np.zeros((0, 4), F), g.ms, g.corner[:40], g.surf[:100], (IDENTITY,))
    if name == "empty_surf":
        return Case(name, g.mc, np.zeros((0, 4), F), g.corner[:40], g.surf[:100], (IDENTITY,))
    raise KeyError(name)


def rod_box(axis, length):
    """The f32 bounding box of a rod: 2 m across, `length` along `axis`, deliberately not round and not centred."""
    lo = np.array([-1.3, 0.7, -0.4], F)
    hi = (lo + F(2.0)).astype(F)
    lo[axis] = F(-0.37 * length - 0.123)
    hi[axis] = F(lo[axis] + F(length))
    return lo, hi


def _snap(rng, v, descs, axis, frac_mask):
    """Move v[frac_mask] (coordinates along `axis`) onto computed cell boundaries of `descs` (alternating), 0-2 f32 steps off."""
    v = v.copy()
    idx = np.flatnonzero(frac_mask)
    for j, g in enumerate(descs):
        sel = idx[j::len(descs)]
        if len(sel) == 0:
            continue
        inv = g.inv_x if axis == 0 else g.inv
        u = gm.u_of(v[sel], g.o[axis], inv).astype(np.float64)
        c = np.where(rng.random(len(sel)) < 0.5, np.floor(u), np.floor(u) + 1)       # a boundary of the value's own cell
        c = np.clip(c, 1, g.dims[axis] - 2)
        above, below = gm.boundary_values(g.o[axis], inv, c)
        up = rng.random(len(sel)) < 0.5
        w = np.where(up, above, below)
        steps = rng.integers(0, 3, len(sel))
        for k in (1, 2):
            w = np.where(steps >= k, np.nextafter(w, np.where(up, F(np.inf), F(-np.inf))), w)
        near = np.abs(w.astype(np.float64) - v[sel]) < 1.0                            # grown cells: only a boundary inside the cluster
        v[sel] = np.where(near, w, v[sel])
    return v


def _rod(name, rng):
    axis, length = RODS[name]
    lo, hi = rod_box(axis, length)
    b = 1 - axis                                                                      # the other horizontal axis
    descs = [gm.grid_desc(lo, hi, max_dim=None), gm.grid_desc(lo, hi)]
    ms, mc, surf, corner = [lo[None], hi[None]], [lo[None], hi[None]], [], []       # the two anchors fix the bounding box
    for start in (float(lo[axis]), float(lo[axis]) + 0.43 * length, float(hi[axis]) - 2.0):
        c0 = lo.astype(np.float64); c0[axis] = start
        # two planes through the cluster's centre, both tilted 45 degrees against the rod: their points spread along the rod (the
        # five neighbours of a query straddle its cell boundaries), and the reference's plane fit n . p = -1 stays well
        # conditioned kilometres from the origin (a plane that nearly contains the origin's direction does not)
        e = np.eye(3)
        patches = []
        for other, e2 in ((e[b], e[2]), (e[2], e[b])):
            nrm, e1 = (e[axis] + other) / np.sqrt(2.0), (e[axis] - other) / np.sqrt(2.0)
            st = rng.uniform(-1, 1, (150, 2))
            patches.append(c0 + 1.0 + st[:, :1] * e1 + st[:, 1:] * e2 + rng.normal(0, 0.004, (150, 1)) * nrm)
        cl = np.concatenate(patches).astype(F)
        cl[:, axis] = _snap(rng, cl[:, axis], descs, axis, rng.random(300) < 1 / 3)
        cl = np.clip(cl, lo, hi)
        ms.append(cl)
        t = rng.uniform(0, 2, 40)
        along = np.repeat(c0[None], 40, 0); along[:, axis] += t; along[:, b] += 0.6; along[:, 2] += 1.1
        up = np.repeat(c0[None], 40, 0); up[:, 2] += t; up[:, axis] += 1.2; up[:, b] += 1.4
        segs = (np.concatenate([along, up]) + rng.normal(0, 0.003, (80, 3))).astype(F)
        mc.append(np.clip(segs, lo, hi))
        sq = (cl[rng.integers(0, 300, 60)] + rng.normal(0, 0.1, (60, 3))).astype(F)
        sq[:, axis] = _snap(rng, sq[:, axis], descs, axis, np.arange(60) < 20)
        surf.append(sq)
        corner.append((segs[rng.integers(0, 80, 12)] + rng.normal(0, 0.05, (12, 3))).astype(F))
    return Case(name, pts4(np.concatenate(mc)), pts4(np.concatenate(ms)), pts4(np.concatenate(corner)), pts4(np.concatenate(surf)),
                (IDENTITY, SHIFT))


def _gate_reach(rng):
    n = 330
    ms, surf = [], []
    for a in range(3):
        for j in range(n):
            q = np.array([7.0 + 3.0 * (j % 20), 31.0 + 3.0 * (j // 20), 5.0 + 3.0 * a])       # groups 3 m apart: no other neighbour
            q[a] += 0.0031 * j                                                                   # the phase against the cell grid
            grp = np.repeat(q[None], 5, 0) + rng.uniform(-0.02, 0.02, (5, 3))
            grp[:, a] = q[a] + (0.995 if j % 2 else -0.995) + rng.uniform(-0.0005, 0.0005, 5)
            ms.append(grp); surf.append(q)
    ms = np.concatenate(ms)
    seg = _segments(rng, ms.min(0), ms.max(0) - ms.min(0), 3, 40, 0.005)
    corner = seg[rng.integers(0, len(seg), 30)] + rng.normal(0, 0.1, (30, 3))
    return Case("gate_reach", pts4(seg), pts4(ms), pts4(corner), pts4(np.array(surf)), (IDENTITY,))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(1001 + NAMES.index(name))
    if name == "generic":
        c = _generic(rng)
    elif name == "lattice":
        c = _lattice(rng)
    elif name == "faces":
        c = _faces(rng)
    elif name in RODS:
        c = _rod(name, rng)
    elif name == "gate_reach":
        c = _gate_reach(rng)
    else:
        c = _degenerate(name, rng)
    for a in (c.mc, c.ms, c.corner, c.surf):
        a.setflags(write=False)
    return c


def with_non_finite(rng, cloud, every=7):
    """`cloud` with a NaN or Inf point inserted after every `every`-th point (in one, two or all three coordinates): the index
    must skip them, and a returned neighbour index must still address the right point."""
    out = []
    for i, p in enumerate(np.asarray(cloud, F)):
        out.append(p)
        if i % every == every - 1:
            bad = p.copy()
            bad[rng.integers(0, 3, rng.integers(1, 4))] = rng.choice([np.nan, np.inf, -np.inf])
            out.append(bad)
    return np.ascontiguousarray(np.array(out, F))
