"""CPU model of msfl_score_poses (msf_loam_amd/csrc/msfl_score.cuh), restated in numpy with explicit f32 / f64 types.

TEST INFRASTRUCTURE, shared by tests/test_score_model.py (CPU) and tests/test_gpu_score.py.  Nothing here touches the GPU.

The model IS the specification: per pose and feature, the nearest map point of the feature's kind in the total order (f32
L2_Simple distance, original map index) among those with d2 <= thr = f32(max_dist^2); inliers are counted and
rint(d2 * 2^32) is summed in integers, per kind.  The GPU is compared with array_equal, no tolerance anywhere.
"""
import numpy as np

from tests import knn_grid_model as gm

F = np.float32
BAD_ARG = 3
DTYPE = np.dtype([("inliers", np.int32, (2,)), ("sum_sq_q32", np.uint64, (2,)), ("status", np.int32), ("reserved_", np.int32)])
Q32 = 4294967296.0


def threshold(max_dist):
    """thr = (float)(max_dist * max_dist), the product in double."""
    return F(np.float64(max_dist) * np.float64(max_dist))


def transform_point_f32(pose, p):
    """msfl_math.cuh transform_point_f32, op for op in float64 (no contraction), then the cast: p (n, 3) f32 -> (n, 3) f32."""
    pose = np.asarray(pose, np.float64)
    t, (qx, qy, qz, qw) = pose[:3], pose[3:]
    v = np.asarray(p, F).astype(np.float64)
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx        # cross(q.vec, v)
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        cx, cy, cz = qy * uz - qz * uy, qz * ux - qx * uz, qx * uy - qy * ux        # cross(q.vec, uv)
        r = np.stack([(vx + qw * ux) + cx, (vy + qw * uy) + cy, (vz + qw * uz) + cz], 1)
        return (r + t).astype(F)


def fixed_point(d2):
    """rint(d2 * 2^32) as Python ints: the scaling is exact in f32 (d2 <= 64), rint is round-to-nearest-even."""
    d2 = np.asarray(d2, F)
    return [int(x) for x in np.rint(d2 * F(Q32)).astype(np.float64)]


MARGIN = 1e-5        # relative; the f32 distance of a pair of f32 points is within 3e-7 of the exact one


def _slow(m, idx, q, thr):
    """One query against the candidates idx (ascending original indices): the first minimum is the lowest index on a tie."""
    d = gm.l2_simple(m[idx], q)
    k = int(np.argmin(d))
    return (d[k], idx[k]) if d[k] <= thr else (F(np.inf), -1)


def nearest(map_pts, q, thr, tree=None, max_dist=None):
    """For every query q (n, 3) f32: (d2, nn) of its nearest map point (original index) with d2 <= thr, in the order (f32
    distance, index); (+inf, -1) without one or for a non-finite query.  Without `tree`: brute force over the whole map.
    `tree` (make_tree) only pre-selects: the candidates within 1.01 * max_dist of a query, and among them a nearest point that
    the f64 distances put clearly (MARGIN) ahead of the second and clearly on one side of max_dist, which no f32 rounding can
    reverse.  Every other query (ties, duplicates, the gate) goes through all its candidates.  The f32 distances decide."""
    m = np.asarray(map_pts, F).reshape(-1, 4)[:, :3]
    q = np.asarray(q, F)
    d2_out, nn_out = np.full(len(q), np.inf, F), np.full(len(q), -1, np.int32)
    ok = np.flatnonzero(np.isfinite(q).all(1))
    if tree is None:
        fin = np.flatnonzero(np.isfinite(m).all(1))
        for i in ok if len(fin) else ():
            d2_out[i], nn_out[i] = _slow(m, fin, q[i], thr)
        return d2_out, nn_out
    kd, kd_idx = tree
    if len(ok) == 0:
        return d2_out, nn_out
    q64 = q[ok].astype(np.float64)
    d, j = kd.query(q64, k=2, distance_upper_bound=1.01 * float(max_dist), workers=4)
    clear = d[:, 0] * (1.0 + MARGIN) < d[:, 1]
    hit = clear & (d[:, 0] <= float(max_dist) * (1.0 - MARGIN))
    miss = np.isinf(d[:, 0]) | (d[:, 0] >= float(max_dist) * (1.0 + MARGIN))
    nn_hit = kd_idx[j[hit, 0]]
    d2_out[ok[hit]], nn_out[ok[hit]] = gm.l2_simple(m[nn_hit], q[ok[hit]]), nn_hit
    rest = np.flatnonzero(~hit & ~miss)
    for r, cand in zip(rest, kd.query_ball_point(q64[rest], 1.01 * float(max_dist)) if len(rest) else ()):
        if len(cand):
            d2_out[ok[r]], nn_out[ok[r]] = _slow(m, np.sort(kd_idx[np.asarray(cand)]), q[ok[r]], thr)
    return d2_out, nn_out


def make_tree(map_pts):
    """(cKDTree over the finite points of a map cloud, their original indices) for `nearest`; None for a cloud without any."""
    from scipy.spatial import cKDTree
    m = np.asarray(map_pts, F).reshape(-1, 4)[:, :3]
    fin = np.flatnonzero(np.isfinite(m).all(1))
    if len(fin) == 0:
        return None
    return cKDTree(m[fin].astype(np.float64)), fin


class Model:
    """The maps of one msfl_set_map, with their candidate trees built once."""

    def __init__(self, map_corner, map_surf, use_tree=True):
        self.maps = (np.asarray(map_corner, F).reshape(-1, 4), np.asarray(map_surf, F).reshape(-1, 4))
        self.trees = tuple(make_tree(m) for m in self.maps) if use_tree else (None, None)
        self.use_tree = use_tree

    def _nearest(self, kind, q, thr, max_dist):
        if self.use_tree:
            if self.trees[kind] is None:
                return np.full(len(q), np.inf, F), np.full(len(q), -1, np.int32)
            return nearest(self.maps[kind], q, thr, self.trees[kind], max_dist)
        return nearest(self.maps[kind], q, thr)

    def score(self, corner, surf, poses, max_dist, want_nn=False):
        """Handle.score_poses: records (P,) of DTYPE, and with want_nn (d2 (P, F) f32, nn (P, F) i32)."""
        corner, surf = np.asarray(corner, F).reshape(-1, 4), np.asarray(surf, F).reshape(-1, 4)
        poses = np.asarray(poses, np.float64).reshape(-1, 7)
        thr = threshold(max_dist)
        rec = np.zeros(len(poses), DTYPE)
        nf = len(corner) + len(surf)
        d2_all, nn_all = np.full((len(poses), nf), np.inf, F), np.full((len(poses), nf), -1, np.int32)
        for h, pose in enumerate(poses):
            if not np.isfinite(pose).all():
                rec["status"][h] = BAD_ARG
                continue
            at = 0
            for kind, feat in enumerate((corner, surf)):
                fin = np.isfinite(feat[:, :3]).all(1)
                q = transform_point_f32(pose, feat[:, :3])
                q[~fin] = np.nan
                d2, nn = self._nearest(kind, q, thr, max_dist)
                hit = nn >= 0
                rec["inliers"][h, kind] = int(hit.sum())
                rec["sum_sq_q32"][h, kind] = sum(fixed_point(d2[hit]))
                d2_all[h, at:at + len(feat)], nn_all[h, at:at + len(feat)] = d2, nn
                at += len(feat)
        return (rec, d2_all, nn_all) if want_nn else rec


def fitness(rec, n_features):
    return rec["inliers"].sum(-1) / float(n_features)


# ---- the walk of msfl_score.cuh nn1_grid, restated: what its row and end-cell tests may skip ------------------------------------

class WalkIndex:
    """The map index of one cloud as the device builds it: descriptor (knn_grid_model.grid_desc), the points of every cell."""

    def __init__(self, map_pts, cap=gm.DEFAULT_CAP, radius=1.0):
        self.m = np.asarray(map_pts, F).reshape(-1, 4)[:, :3]
        self.g = gm.desc_of(map_pts, cap, radius=radius)
        self.cells = {}
        fin = np.flatnonzero(np.isfinite(self.m).all(1))
        if len(fin):
            dx, dy, dz = self.g.dims
            pc = gm.point_cell(self.m[fin], self.g)
            for i, c in zip(fin, (pc[:, 2] * dy + pc[:, 1]) * dx + pc[:, 0]):
                self.cells.setdefault(int(c), []).append(int(i))


def walk_nearest(ix, q, thr):
    """nn1_grid for ONE finite query q (3,) f32: (d2, nn, candidates evaluated).  Rows in the kernel's order; a row or end cell is
    skipped when its lower bound exceeds the current best distance; (distance, index) keys."""
    g = ix.g
    dx, dy, dz = g.dims
    if not ix.cells:
        return F(np.inf), -1, 0
    u = [gm.u_of(q[0], g.o[0], g.inv_x), gm.u_of(q[1], g.o[1], g.inv), gm.u_of(q[2], g.o[2], g.inv)]
    cx, cy, cz = (int(gm.grid_coord(q[a], g.o[a], g.inv_x if a == 0 else g.inv, g.dims[a])) for a in range(3))
    xs, xe = max(cx - gm.XSUB, 0), min(cx + gm.XSUB, dx - 1)
    best = (F(thr), 0xffffffff)
    n_cand = 0
    if xs > xe:
        return F(np.inf), -1, 0
    gap = lambda a, c: F(gm.axis_gap(u[a], np.int64(c)))
    gy = {o: gap(1, cy + o) for o in (-1, 0, 1)}
    gz = {o: gap(2, cz + o) for o in (-1, 0, 1)}
    gxa = [F(F(gap(0, xs + k) * gap(0, xs + k)) * g.cellx2) for k in range(gm.XSUB)]
    gxb = [F(F(gap(0, xe - k) * gap(0, xe - k)) * g.cellx2) for k in range(gm.XSUB)]
    sy, sz = (-1 if gy[-1] <= gy[1] else 1), (-1 if gz[-1] <= gz[1] else 1)
    g_ny, g_fy, g_nz, g_fz = gy[sy], gy[-sy], gz[sz], gz[-sz]
    near = [(sy, 0), (0, sz)] if g_ny <= g_nz else [(0, sz), (sy, 0)]
    far = [(-sy, 0), (0, -sz)] if g_fy <= g_fz else [(0, -sz), (-sy, 0)]
    mixed = [(sy, -sz), (-sy, sz)] if F(g_ny * g_ny) + F(g_fz * g_fz) <= F(g_fy * g_fy) + F(g_nz * g_nz) else [(-sy, sz), (sy, -sz)]
    for oy, oz in [(0, 0)] + near + far + [(sy, sz)] + mixed + [(-sy, -sz)]:
        y, z = cy + oy, cz + oz
        if y < 0 or y >= dy or z < 0 or z >= dz:
            continue
        row2 = F(F(F(gy[oy] * gy[oy]) + F(gz[oz] * gz[oz])) * g.cell2)
        if row2 > best[0]:
            continue
        a, b, da, db = xs, xe, True, True
        for k in range(gm.XSUB):
            da = da and bool(F(row2 + gxa[k]) > best[0]); a += int(da)
            db = db and bool(F(row2 + gxb[k]) > best[0]); b -= int(db)
        for c in range(a, b + 1):
            for i in ix.cells.get((z * dy + y) * dx + c, ()):
                n_cand += 1
                best = min(best, (gm.l2_simple(ix.m[i], q), i))
    return (best[0], best[1], n_cand) if best[1] != 0xffffffff else (F(np.inf), -1, n_cand)
