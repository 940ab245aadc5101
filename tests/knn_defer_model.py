"""CPU model of the 5-NN walk of knn5_grid_k32 (msf_loam_amd/csrc/msfl_knn_index.cuh) with its DEFER form: capped row visits, the
rest of a long range pushed on a per-lane stack and walked after the ninth row.  Built on tests/knn_grid_model.py (descriptor,
cell coordinates, axis_gap: all f32 as on the device).

TEST INFRASTRUCTURE, shared by tests/test_knn_defer_model.py and tools/sim/knn_defer_model.py.  Nothing here touches the GPU.

The model keeps the exact top five by (f32 distance, map index) and prunes on the exact 5th distance.  The device prunes on a
bound that is never below it (the truncated key | 7), so it visits what the model visits or more: no miss here, no miss there.
"""
import numpy as np

from tests import knn_grid_model as gm

F = np.float32
SHIPPED_CAPS = (8, 4, 4, 1, 1, 1, 1, 1, 1)       # MSFL_KNN_DEFER_CAPS: pair-iterations per row position, in visit order
SHIPPED_DEPTH = 4                                 # MSFL_KNN_DEFER_DEPTH
NO_DEFER = None


class Index:
    """The sorted copy and cell table of one map cloud under descriptor g (grid_count / grid_scatter; non-finite points are left out)."""

    def __init__(self, cloud, g):
        p = np.asarray(cloud, F).reshape(-1, 4)[:, :3]
        keep = np.flatnonzero(np.isfinite(p).all(1))
        pc = gm.point_cell(p[keep], g) if len(keep) else np.zeros((0, 3), np.int64)
        dx, dy, dz = g.dims
        key = (pc[:, 2] * dy + pc[:, 1]) * dx + pc[:, 0]
        order = np.argsort(key, kind="stable")
        self.g = g
        self.orig = keep[order]                      # sorted position -> index in the cloud
        self.pts = p[self.orig]
        self.start = np.searchsorted(key[order], np.arange(g.n_cells + 1)).tolist()


def setup(ix, q):
    """The walk's set-up for the queries q (n, 3), vectorised: per query the nine rows in visit order (valid, first cell index of the
    row, squared row bound), the x reach and the monotone end-cell bounds.  Lists of Python floats / ints (f32 values are exact in f64)."""
    g = ix.g
    q = np.asarray(q, F).reshape(-1, 3)
    dx, dy, dz = g.dims
    ux, uy, uz = gm.u_of(q[:, 0], g.o[0], g.inv_x), gm.u_of(q[:, 1], g.o[1], g.inv), gm.u_of(q[:, 2], g.o[2], g.inv)
    cx, cy, cz = gm.grid_coord(q[:, 0], g.o[0], g.inv_x, dx), gm.grid_coord(q[:, 1], g.o[1], g.inv, dy), gm.grid_coord(q[:, 2], g.o[2], g.inv, dz)
    xs, xe = np.maximum(cx - gm.XSUB, 0), np.minimum(cx + gm.XSUB, dx - 1)
    gxa, gxb = [], []
    for k in range(gm.XSUB):
        ga, gb = gm.axis_gap(ux, xs + k), gm.axis_gap(ux, xe - k)
        gxa.append(np.where(xs + k < cx, ga * ga * g.cellx2, F(0.0)).astype(F))
        gxb.append(np.where(xe - k > cx, gb * gb * g.cellx2, F(0.0)).astype(F))
    gy0, gy1, gy2 = gm.axis_gap(uy, cy - 1), gm.axis_gap(uy, cy), gm.axis_gap(uy, cy + 1)
    gz0, gz1, gz2 = gm.axis_gap(uz, cz - 1), gm.axis_gap(uz, cz), gm.axis_gap(uz, cz + 1)
    y_lo, z_lo = gy0 <= gy2, gz0 <= gz2
    sy, sz = np.where(y_lo, -1, 1), np.where(z_lo, -1, 1)
    g_ny, g_fy = np.where(y_lo, gy0, gy2), np.where(y_lo, gy2, gy0)
    g_nz, g_fz = np.where(z_lo, gz0, gz2), np.where(z_lo, gz2, gz0)
    ny_first, fy_first = g_ny <= g_nz, g_fy <= g_fz
    q_ny, q_fy, q_nz, q_fz, q_y1, q_z1 = g_ny * g_ny, g_fy * g_fy, g_nz * g_nz, g_fz * g_fz, gy1 * gy1, gz1 * gz1
    e_first = q_ny + q_fz <= q_fy + q_nz
    zero = np.zeros_like(sy)

    def pick(first, a, b):
        return np.where(first, a, b), np.where(first, b, a)
    rows = [(zero, zero, q_y1 + q_z1)]
    for first, (ay, az, ra), (by, bz, rb) in ((ny_first, (sy, zero, q_ny + q_z1), (zero, sz, q_y1 + q_nz)),
                                              (fy_first, (-sy, zero, q_fy + q_z1), (zero, -sz, q_y1 + q_fz))):
        y1, y2 = pick(first, ay, by); z1, z2 = pick(first, az, bz); r1, r2 = pick(first, ra, rb)
        rows += [(y1, z1, r1), (y2, z2, r2)]
    rows.append((sy, sz, q_ny + q_nz))
    y1, y2 = pick(e_first, sy, -sy); z1, z2 = pick(e_first, -sz, sz); r1, r2 = pick(e_first, q_ny + q_fz, q_fy + q_nz)
    rows += [(y1, z1, r1), (y2, z2, r2)]
    rows.append((-sy, -sz, q_fy + q_fz))
    valid, base, row2 = [], [], []
    for oy, oz, rq in rows:
        y, z = cy + oy, cz + oz
        valid.append(((y >= 0) & (y < dy) & (z >= 0) & (z < dz)).tolist())
        base.append(((z * dy + y) * dx).tolist())
        row2.append((rq.astype(F) * g.cell2).astype(F).tolist())
    return {"n": len(q), "xs": xs.tolist(), "xe": xe.tolist(), "gxa": [a.tolist() for a in gxa], "gxb": [b.tolist() for b in gxb],
            "valid": valid, "base": base, "row2": row2}


def walk(ix, su, i, d2, gate=1.0, caps=NO_DEFER, depth=SHIPPED_DEPTH, trace=False):
    """Query i of set-up su; d2: its f32 distances to ix.pts (an f32 array; with trace=True a list of floats).  Returns (top, stats): top = the up to five smallest
    (distance, cloud index) offered, sorted; stats = candidates evaluated, ranges deferred, ranges walked in place because the
    stack was full, rows visited, and with trace=True `iters`: per row position the per-pair-iteration insertion flags (bit 0 / 1:
    the first / second candidate passed the pre-filter) and `tails`: the same per deferred range."""
    top = []
    orig = ix.orig
    st = {"cand": 0, "deferred": 0, "in_place": 0, "visited": 0, "iters": [[] for _ in range(9)], "tails": []}
    xs, xe = su["xs"][i], su["xe"][i]
    if xs > xe:
        return top, st
    start = ix.start
    stack = []

    def run(s, e, log):
        st["cand"] += e - s
        if not trace:
            # only what passes the pre-filter at the range's start can pass it later: the bound never grows
            seg = d2[s:e]
            hit = np.flatnonzero(seg <= (top[4][0] if len(top) == 5 else gate))
            for k, d in zip(hit.tolist(), seg[hit].tolist()):
                key = (d, int(orig[s + k]))
                if len(top) < 5:
                    top.append(key); top.sort()
                elif key < top[4]:
                    top[4] = key; top.sort()
            return
        k = s
        while k < e:
            flags = 0
            for j in (0, 1):
                if k + j < e:
                    d = d2[k + j]
                    bound = top[4][0] if len(top) == 5 else gate
                    if d <= bound:                       # the pre-filter
                        flags |= 1 << j
                        key = (d, int(orig[k + j]))
                        if len(top) < 5 or key < top[4]:
                            top.append(key); top.sort(); del top[5:]
            if trace:
                log.append(flags)
            k += 2

    for pos in range(9):
        row2 = su["row2"][pos][i]
        d4 = top[4][0] if len(top) == 5 else gate
        if not su["valid"][pos][i] or row2 > d4:
            continue
        room = float(F(d4) - F(row2))
        a, b = xs, xe
        for k in range(gm.XSUB):
            a += su["gxa"][k][i] > room
            b -= su["gxb"][k][i] > room
        if a > b:
            continue
        row = su["base"][pos][i]
        s, e = start[row + a], start[row + b + 1]
        if s == e:
            continue
        st["visited"] += 1
        if caps is not None and e - s > 2 * caps[pos]:
            if len(stack) < depth:
                stack.append((s + 2 * caps[pos], e))
                st["deferred"] += 1
                e = s + 2 * caps[pos]
            else:
                st["in_place"] += 1
        run(s, e, st["iters"][pos])
    for s, e in stack:                                   # stack order
        log = []
        run(s, e, log)
        st["tails"].append(log if trace else (e - s + 1) // 2)
    return top, st


def brute_top5(ix, d2, gate=1.0):
    """The five smallest (distance, cloud index) among the indexed points within the gate."""
    d = np.asarray(d2, F)
    cand = np.flatnonzero(d <= F(gate))
    keys = sorted((float(d[k]), int(ix.orig[k])) for k in cand)
    return keys[:5]


def wave_stats(lanes, flat=True):
    """lanes: the traced stats of the (up to 64) queries of one wavefront.  Returns pair-iterations (row visits + overflow), wave-level
    insertion passes, visited positions, the most deferred ranges of a lane."""
    trips = passes = visited = 0

    def level(logs):                                     # logs: one flag list per lane, walked side by side
        n = max((len(l) for l in logs), default=0)
        p = 0
        for j in range(n):
            f = 0
            for l in logs:
                if j < len(l):
                    f |= l[j]
            p += (f & 1) + (f >> 1)
        return n, p
    for pos in range(9):
        n, p = level([s["iters"][pos] for s in lanes])
        trips += n; passes += p; visited += n > 0
    if flat:
        n, p = level([[f for t in s["tails"] for f in t] for s in lanes])
        trips += n; passes += p
    else:
        for k in range(max((len(s["tails"]) for s in lanes), default=0)):
            n, p = level([s["tails"][k] for s in lanes if len(s["tails"]) > k])
            trips += n; passes += p
    return trips, passes, visited, max((len(s["tails"]) for s in lanes), default=0)
