"""CPU model of the scan-to-map 5-NN index geometry (msf_loam_amd/csrc/msfl_kernels.cuh: grid_desc_from_bbox, grid_coord,
axis_gap and the row / end-cell skipping rule of knn5_grid and knn5_grid_k32), restated in numpy with explicit f32 / f64 types.

TEST INFRASTRUCTURE, shared by tests/test_knn_grid_model.py (CPU) and tests/test_gpu_knn_grid.py (which only takes the
descriptor from it, to say which cap grows which map).  Nothing here touches the GPU.

The one question the model answers: given a query, one of its true five nearest map points and the true 5th distance d4, may
the walk leave that point's cell unvisited?  The walk only ever compares a LOWER BOUND of a row or end cell against its
current 5th distance, which is never below the final one, so "bound > d4" is the most any visit order can skip.
"""
import collections

import numpy as np

F = np.float32
XSUB = 3                      # MSFL_GRID_XSUB / kGridXSub
SLACK = F(1e-3)               # axis_gap: every lower bound is shrunk by this many cells
EDGE_MARGIN = 1.001           # base cell edge = EDGE_MARGIN * acceptance radius
GROWTH = 1.26                 # growth step of the cell edge
MAX_DIM = 4096                # kGridMaxDim
CAPS = (8, 64, 4096, 65536, 1 << 20, 64 << 20)
DEFAULT_CAP = 1 << 20         # span of a handle's first build

Desc = collections.namedtuple("Desc", "o inv inv_x dims n_cells want_cells cell2 cellx2 cell steps")


def squares(inv, inv_x):
    """grid_desc_squares: (1 / inv)^2 in f32."""
    cell, cellx = F(1.0) / F(inv), F(1.0) / F(inv_x)
    return F(cell * cell), F(cellx * cellx)


def grid_desc(mn, mx, radius=1.0, cap=DEFAULT_CAP, max_dim=MAX_DIM):
    """grid_desc_from_bbox.  mn / mx: the f32 bounding box (None: no finite point).  max_dim=None is the descriptor without
    the per-axis limit (what the code did before kGridMaxDim)."""
    if mn is None:
        c2, cx2 = squares(F(1.0), F(XSUB))
        return Desc(np.zeros(3, F), F(1.0), F(XSUB), (1, 1, 1), 1, 1, c2, cx2, 1.0, 0)
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    cell = EDGE_MARGIN * float(radius)                    # f64 from here on
    want, steps = None, 0
    while True:
        dims, total = [], 1.0
        for a in range(3):
            edge = cell / XSUB if a == 0 else cell
            d = int(np.floor((float(mx[a]) - float(mn[a])) / edge)) + 2
            dims.append(max(d, 2))
            total *= dims[-1]
        if want is None:
            want = int(total) if total < 2.0e9 else 2000000000
        if total <= float(cap) and (max_dim is None or max(dims) <= max_dim):
            break
        cell *= GROWTH
        steps += 1
    inv, inv_x = F(1.0 / cell), F(float(XSUB) / cell)
    c2, cx2 = squares(inv, inv_x)
    return Desc(mn.copy(), inv, inv_x, tuple(dims), dims[0] * dims[1] * dims[2], want, c2, cx2, cell, steps)


def bbox_of(pts):
    """grid_bbox_body: min / max over the points whose three coordinates are finite."""
    p = np.asarray(pts, F).reshape(-1, 4)[:, :3]
    p = p[np.isfinite(p).all(1)]
    return (None, None) if len(p) == 0 else (p.min(0), p.max(0))


def desc_of(pts, cap=DEFAULT_CAP, max_dim=MAX_DIM, radius=1.0):
    return grid_desc(*bbox_of(pts), radius=radius, cap=cap, max_dim=max_dim)


def u_of(v, o, inv):
    """The f32 cell coordinate fl(fl(v - o) * inv)."""
    return (np.asarray(v, F) - F(o)) * F(inv)


def grid_coord(v, o, inv, dim):
    """grid_coord: floor, clamped in float to [-2, dim + 1]."""
    u = np.floor(u_of(v, o, inv))
    return np.minimum(np.maximum(u, F(-2.0)), F(dim) + F(1.0)).astype(np.int64)


def point_cell(p, g):
    """Cell of a map point (grid_count_body): grid_coord clamped to [0, dim - 1], per axis.  p: (n, 3)."""
    p = np.asarray(p, F)
    out = []
    for a, inv in enumerate((g.inv_x, g.inv, g.inv)):
        c = grid_coord(p[:, a], g.o[a], inv, g.dims[a])
        out.append(np.clip(c, 0, g.dims[a] - 1))
    return np.stack(out, 1)


def axis_gap(u, c):
    """axis_gap: distance in cells from u to [c, c + 1], minus the slack, floored at 0; all f32."""
    c = np.asarray(c)
    g = np.maximum(c.astype(F) - u, u - (c + 1).astype(F))
    return np.maximum(g - SLACK, F(0.0))


def l2_simple(a, q):
    """f32 squared distance in FLANN L2_Simple order."""
    d = np.asarray(a, F) - np.asarray(q, F)
    r = d[..., 0] * d[..., 0]
    r = r + d[..., 1] * d[..., 1]
    return r + d[..., 2] * d[..., 2]


def may_skip(g, q, p, d4):
    """Pairs (q[i], p[i]) of a query and one of its true top five, d4[i] the true 5th distance (f32).  Returns a dict of boolean
    arrays: `reach` (the point's cell lies outside the 27-cell, 2 * XSUB + 1 wide neighbourhood), `row` (its (y, z) row may be
    skipped), `end` (its cell may be trimmed off the end of the row, by either walk's form of the test), `any`, and `margin`:
    sqrt(d4) - sqrt(bound) in cells for the tightest positive bound that applied to the point's cell (negative = a miss)."""
    q, p, d4 = np.asarray(q, F), np.asarray(p, F), np.asarray(d4, F)
    dx, dy, dz = g.dims
    pc = point_cell(p, g)
    ux, uy, uz = u_of(q[:, 0], g.o[0], g.inv_x), u_of(q[:, 1], g.o[1], g.inv), u_of(q[:, 2], g.o[2], g.inv)
    cx, cy, cz = grid_coord(q[:, 0], g.o[0], g.inv_x, dx), grid_coord(q[:, 1], g.o[1], g.inv, dy), grid_coord(q[:, 2], g.o[2], g.inv, dz)
    xs, xe = np.maximum(cx - XSUB, 0), np.minimum(cx + XSUB, dx - 1)
    reach = (np.abs(pc[:, 1] - cy) > 1) | (np.abs(pc[:, 2] - cz) > 1) | (pc[:, 0] < xs) | (pc[:, 0] > xe)
    gy, gz = axis_gap(uy, pc[:, 1]), axis_gap(uz, pc[:, 2])
    row2 = (gy * gy + gz * gz) * g.cell2
    row = row2 > d4
    # end cells: knn5_grid drops the leading run of cells with row2 + gx > d4 on each side (at most XSUB of them), knn5_grid_k32
    # counts the cells on the query's outer side with gx > d4 - row2 (bounds of cells at or beyond the query's own are zeroed)
    room = d4 - row2
    end = np.zeros(len(q), bool)
    bound = row2.copy()
    for side in (0, 1):
        run = np.ones(len(q), bool)
        for k in range(XSUB):
            c = xs + k if side == 0 else xe - k
            ga = axis_gap(ux, c)
            gx = ga * ga * g.cellx2
            run = run & (row2 + gx > d4)
            outer = c < cx if side == 0 else c > cx
            k32 = outer & (gx > room)
            here = pc[:, 0] == c
            end |= here & (run | k32)
            bound = np.where(here & ~reach, np.maximum(bound, row2 + gx), bound)
    # how far, in cells, the tightest bound that applied stays below the 5th distance (inf where no bound was positive)
    with np.errstate(invalid="ignore"):
        margin = np.where(bound > 0, (np.sqrt(d4.astype(np.float64)) - np.sqrt(bound.astype(np.float64))) * float(g.inv), np.inf)
    return {"reach": reach, "row": row & ~reach, "end": end & ~reach & ~row, "any": reach | row | end, "margin": margin,
            "u_max": float(max(np.abs(ux).max(), np.abs(uy).max(), np.abs(uz).max())) if len(q) else 0.0}


def candidates_upper_bound(g, cloud, q, d4):
    """The most candidates knn5_grid_k32 can evaluate for the queries q (n, 3) when its 5th distance starts at d4 (the gate) and
    only ever falls: the points in the cells of each visited row that the end-cell count leaves, with every row and cell tested
    against d4 itself.  Also returns the count with no test at all (the whole clipped neighbourhood).  Any visit order stays
    below the first number; a walk whose bounds ignore the size of its cells approaches the second."""
    q, d4 = np.asarray(q, F), F(d4)
    dx, dy, dz = g.dims
    p = np.asarray(cloud, F).reshape(-1, 4)[:, :3]
    p = p[np.isfinite(p).all(1)]
    pc = point_cell(p, g)
    per_cell = collections.Counter(((pc[:, 2] * dy + pc[:, 1]) * dx + pc[:, 0]).tolist())
    ux, uy, uz = u_of(q[:, 0], g.o[0], g.inv_x), u_of(q[:, 1], g.o[1], g.inv), u_of(q[:, 2], g.o[2], g.inv)
    cx, cy, cz = grid_coord(q[:, 0], g.o[0], g.inv_x, dx), grid_coord(q[:, 1], g.o[1], g.inv, dy), grid_coord(q[:, 2], g.o[2], g.inv, dz)
    xs, xe = np.maximum(cx - XSUB, 0), np.minimum(cx + XSUB, dx - 1)
    gxa, gxb = [], []
    for k in range(XSUB):
        ga, gb = axis_gap(ux, xs + k), axis_gap(ux, xe - k)
        gxa.append(np.where(xs + k < cx, ga * ga * g.cellx2, F(0.0)))
        gxb.append(np.where(xe - k > cx, gb * gb * g.cellx2, F(0.0)))
    bounded = full = 0
    for oy in (-1, 0, 1):
        for oz in (-1, 0, 1):
            y, z = cy + oy, cz + oz
            valid = (y >= 0) & (y < dy) & (z >= 0) & (z < dz) & (xs <= xe)
            gy, gz = axis_gap(uy, y), axis_gap(uz, z)
            row2 = (gy * gy + gz * gz) * g.cell2
            room = d4 - row2
            a, b = xs.copy(), xe.copy()
            for k in range(XSUB):
                a += gxa[k] > room
                b -= gxb[k] > room
            for i in np.flatnonzero(valid):
                row = (int(z[i]) * dy + int(y[i])) * dx
                full += sum(per_cell.get(row + c, 0) for c in range(int(xs[i]), int(xe[i]) + 1))
                if not row2[i] > d4:
                    bounded += sum(per_cell.get(row + c, 0) for c in range(int(a[i]), int(b[i]) + 1))
    return bounded, full


# ---- the adversarial search --------------------------------------------------------------------------------------------------

def _ordered(v):
    """float_to_ordered: an integer key in the order of the f32 values."""
    i = np.asarray(v, F).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7fffffff)


def _from_ordered(k):
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k, k ^ 0x7fffffff).astype(np.int32).view(F)


def boundary_values(o, inv, c):
    """For integer cells c (array): the smallest f32 v with floor(u(v)) >= c and the largest with floor(u(v)) < c: the two sides
    of the COMPUTED cell boundary.  u is monotone in v, so a bisection over the ordered f32 values finds them."""
    o, inv = F(o), F(inv)
    c = np.asarray(c, np.float64)
    v0 = np.float64(o) + c / np.float64(inv)
    pad = 0.01 / float(inv) + 1e-3 * np.abs(v0)
    lo, hi = _ordered((v0 - pad).astype(F)), _ordered((v0 + pad).astype(F))       # u(lo) < c <= u(hi)
    inside = lambda k: np.floor(u_of(_from_ordered(k), o, inv)) >= c.astype(F)
    assert not inside(lo).any() and inside(hi).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        m = inside(mid)
        hi, lo = np.where(m, mid, hi), np.where(m, lo, mid)
    return _from_ordered(hi), _from_ordered(lo)


def adversarial(g, axis, u_lo, u_hi, n, rng):
    """n trials on one axis of descriptor g, cells drawn from [u_lo, u_hi].  A map point sits on a computed cell boundary (the
    first f32 of cell c, or the last of cell c - 1, a few steps off it for a part of the trials); the query lies on the other
    side at a distance drawn so that the point's row (y axis) or end cell (x axis) lower bound is within a few ulp of the
    point's own distance; the other two coordinates are equal.  d4 is the point's own f32 distance: the point is the 5th
    neighbour, or tied with it.  Returns (misses, smallest margin in cells, largest |u|): a miss is a pair inside the gate whose
    cell the model's walk may skip or cannot reach."""
    inv = g.inv_x if axis == 0 else g.inv
    o = g.o[axis]
    c = rng.integers(int(u_lo), int(u_hi) + 1, n)
    above, below = boundary_values(o, inv, c)
    up = rng.random(n) < 0.5                                  # the point is the first value of cell c, the query below it
    vp = np.where(up, above, below)
    steps = rng.integers(0, 3, n)                             # 0, 1 or 2 f32 steps further into the point's own cell
    for k in (1, 2):
        vp = np.where(steps >= k, np.nextafter(vp, np.where(up, F(np.inf), F(-np.inf))), vp)
    reach_cells = float(XSUB) if axis == 0 else 1.0
    edge = 1.0 / float(inv)
    kind = rng.integers(0, 3, n)
    # distances: anywhere inside the gate; just inside the gate; and within the neighbourhood's last cell
    delta = np.where(kind == 0, rng.uniform(0.0, 1.0, n),
                     np.where(kind == 1, 1.0 - np.abs(rng.normal(0, 2e-3, n)), rng.uniform(min(0.9, (reach_cells - 1.0) * edge), 1.0, n)))
    delta = np.clip(delta, 0.0, 1.0)
    vq = (vp.astype(np.float64) + np.where(up, -delta, delta)).astype(F)
    other = rng.uniform(-1, 1, (n, 2)).astype(F)
    q, p = np.zeros((n, 3), F), np.zeros((n, 3), F)
    # the other two axes: a fixed in-box position shared by query and point
    oth = [a for a in range(3) if a != axis]
    for j, a in enumerate(oth):
        inv_a = g.inv_x if a == 0 else g.inv
        mid = F(g.o[a]) + F(0.4 * min(g.dims[a] - 1, 2) / float(inv_a)) + other[:, j] * F(0.01)
        q[:, a] = mid
        p[:, a] = mid
    q[:, axis], p[:, axis] = vq, vp
    d2 = l2_simple(p, q)
    ok = d2 < F(1.0)                                          # the gate: a neighbour at or past it never matters
    r = may_skip(g, q[ok], p[ok], d2[ok])
    return int(r["any"].sum()), (float(r["margin"].min()) if ok.any() else np.inf), r["u_max"], {k: int(r[k].sum()) for k in ("reach", "row", "end")}
