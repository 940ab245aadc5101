"""numpy model of msfl_segment_scans (docs/kernels/segment.md): every f32 step in the order the kernels take it, every decision an
integer one after that, so the GPU outputs are compared with array_equal.  The components are stated twice, independently: by
hooking + pointer jumping over the edge list (`components_union`) and by a breadth-first flood fill (`components_flood`)."""
from collections import deque
from types import SimpleNamespace

import numpy as np

NONE, SHADOWED, GROUND, SEGMENT, OUTLIER = range(5)
F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

DEFAULTS = dict(n_col=1800, n_row=16, elev_low_deg=-15.0, elev_high_deg=15.0, row_elev_deg=None, min_range=0.3, max_range=100.0,
                ground_rows=8, ground_angle_deg=10.0, up=(0.0, 0.0, 1.0), segment_angle_deg=60.0, min_points=30, min_points_tall=5,
                min_rows_tall=3, keep_classes=(1 << GROUND) | (1 << SEGMENT))


def config(**kw):
    """The fields of msfl_segment_config with the library's defaults; row_elev_deg: None or a sequence of n_row elevations."""
    d = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in d:
            raise TypeError("msfl_segment_config has no field " + k)
        d[k] = v
    return SimpleNamespace(**d)


def elevations_deg(cfg):
    """e[k] in degrees, f64 (the f32 fields of the C struct are widened first)."""
    if cfg.row_elev_deg is not None:
        return np.asarray(cfg.row_elev_deg, F).astype(np.float64)
    lo, hi = float(F(cfg.elev_low_deg)), float(F(cfg.elev_high_deg))
    return np.array([lo + (hi - lo) * k / (cfg.n_row - 1) for k in range(cfg.n_row)])


def tables(cfg):
    """(cc, cs, vs, vc, scalars): the model's own double-then-f32 construction of what msfl_segment_tables returns."""
    k = np.arange(cfg.n_col // 2, dtype=np.float64)
    a = 2.0 * np.pi * (k - 0.5) / cfg.n_col
    e = elevations_deg(cfg)
    step = (e[1:] - e[:-1]) * np.pi / 180.0
    h = 2.0 * np.pi / cfg.n_col
    g = np.sin(float(F(cfg.ground_angle_deg)) * np.pi / 180.0)
    scalars = np.array([np.sin(h), np.cos(h), g * g, np.tan(float(F(cfg.segment_angle_deg)) * np.pi / 180.0)]).astype(F)
    return np.cos(a).astype(F), np.sin(a).astype(F), np.sin(step).astype(F), np.cos(step).astype(F), scalars


def pixels(pts, ring, cfg, tab):
    """(has, r, pix) per point: seg_pixel's steps on f32 arrays (numpy never contracts a multiply and an add)."""
    cc, cs = tab[0], tab[1]
    pts = np.asarray(pts, F).reshape(-1, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    ring = np.asarray(ring).astype(np.int64)
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        rho2 = x * x + y * y
        r = np.sqrt(rho2 + z * z)
        has = finite & (rho2 != 0) & (r >= F(cfg.min_range)) & ~(r > F(cfg.max_range)) & (ring < cfg.n_row)
        half = cfg.n_col // 2
        t0 = cc[0] * y - cs[0] * x
        u0 = cc[0] * x + cs[0] * y
        upper = (t0 > 0) | ((t0 == 0) & (u0 > 0))
        xp, yp = np.where(upper, x, -x), np.where(upper, y, -y)
        lo = np.zeros(len(x), np.int64)
        hi = np.full(len(x), half, np.int64)
        while np.any(hi - lo > 1):
            live = hi - lo > 1
            mid = (lo + hi) >> 1
            ok = cc[mid] * yp - cs[mid] * xp >= 0
            lo = np.where(live & ok, mid, lo)
            hi = np.where(live & ~ok, mid, hi)
    col = lo + np.where(upper, 0, half)
    pix = np.where(has, np.minimum(ring, cfg.n_row - 1) * cfg.n_col + col, -1)
    return has, r, pix


def winners(r, has, pix, npix):
    """key[pixel] = min over the pixel's points of (bits(r) << 32) | index, EMPTY where there is none."""
    key = np.full(npix, EMPTY, np.uint64)
    idx = np.flatnonzero(has)
    k = (r[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    np.minimum.at(key, pix[idx], k)
    return key


def ground_pixels(pts, key, cfg, tab):
    g2 = tab[4][2]
    n_col = cfg.n_col
    ground = np.zeros(cfg.n_col * cfg.n_row, bool)
    if cfg.ground_rows == 0:
        return ground
    lo = np.arange(cfg.ground_rows * n_col)
    hi = lo + n_col
    both = (key[lo] != EMPTY) & (key[hi] != EMPTY)
    lo, hi = lo[both], hi[both]
    a = pts[(key[lo] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    b = pts[(key[hi] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    up = np.asarray(cfg.up, F)
    with np.errstate(all="ignore"):
        dx, dy, dz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
        v = ((up[0] * dx) + (up[1] * dy)) + (up[2] * dz)
        n2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        g = v * v <= g2 * n2
    ground[lo[g]] = True
    ground[hi[g]] = True
    return ground


def edges(key, part, cfg, tab):
    """(a, b) pixel index arrays of the connected pairs: right neighbour (columns wrap) and upper neighbour (rows do not)."""
    vs, vc, (hs, hc, _, t) = tab[2], tab[3], tab[4]
    n_col, n_row = cfg.n_col, cfg.n_row
    rng = (key >> np.uint64(32)).astype(np.uint32).view(F)
    p = np.arange(n_col * n_row)
    row, col = p // n_col, p % n_col

    def connected(a, b, s, c):
        with np.errstate(all="ignore"):
            d1, d2 = np.maximum(rng[a], rng[b]), np.minimum(rng[a], rng[b])
            return d2 * s > t * (d1 - d2 * c)

    q = row * n_col + np.where(col + 1 == n_col, 0, col + 1)
    ok = part[p] & part[q]
    a1, b1 = p[ok], q[ok]
    c1 = connected(a1, b1, hs, hc)
    up = row + 1 < n_row
    pu, qu = p[up], p[up] + n_col
    ok = part[pu] & part[qu]
    a2, b2 = pu[ok], qu[ok]
    c2 = connected(a2, b2, vs[a2 // n_col], vc[a2 // n_col])
    return np.concatenate([a1[c1], a2[c2]]), np.concatenate([b1[c1], b2[c2]])


def components_union(part, ea, eb):
    """label[pixel] = smallest pixel index of its component (-1: takes no part).  Hooking + pointer jumping until nothing moves."""
    n = len(part)
    lab = np.arange(n)
    while True:
        la, lb = lab[ea], lab[eb]
        m = np.minimum(la, lb)
        new = lab.copy()
        np.minimum.at(new, la, m)
        np.minimum.at(new, lb, m)
        while True:
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(part, lab, -1)


def components_flood(part, ea, eb):
    """The same labels by a breadth-first fill from every unvisited pixel in ascending order."""
    n = len(part)
    adj = [[] for _ in range(n)]
    for a, b in zip(ea.tolist(), eb.tolist()):
        adj[a].append(b)
        adj[b].append(a)
    lab = np.full(n, -1, np.int64)
    for s in np.flatnonzero(part).tolist():
        if lab[s] >= 0:
            continue
        lab[s] = s
        todo = deque([s])
        while todo:
            u = todo.popleft()
            for w in adj[u]:
                if lab[w] < 0:
                    lab[w] = s
                    todo.append(w)
    return lab


def segment_scan(pts, ring, cfg, tab=None, method="union"):
    """One scan.  Returns dict(cls u8, segment i32, masked f32 (n, 4), info i32[10]) as msfl_segment_scan delivers them."""
    tab = tables(cfg) if tab is None else tab
    pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 4))
    n = len(pts)
    npix = cfg.n_col * cfg.n_row
    has, r, pix = pixels(pts, ring, cfg, tab)
    key = winners(r, has, pix, npix)
    occupied = key != EMPTY
    ground = ground_pixels(pts, key, cfg, tab)
    part = occupied & ~ground
    ea, eb = edges(key, part, cfg, tab)
    lab = (components_union if method == "union" else components_flood)(part, ea, eb)
    roots = np.flatnonzero(part & (lab == np.arange(npix)))
    count = np.bincount(lab[part], minlength=npix)
    rows_touched = np.zeros(npix, np.int64)
    pr = np.unique(np.stack([lab[part], np.flatnonzero(part) // cfg.n_col], axis=1), axis=0) if part.any() else np.zeros((0, 2), np.int64)
    np.add.at(rows_touched, pr[:, 0], 1)
    valid = (count >= cfg.min_points) | ((count >= cfg.min_points_tall) & (rows_touched >= cfg.min_rows_tall))
    cls = np.zeros(n, np.uint8)
    seg = np.full(n, -1, np.int32)
    idx = np.flatnonzero(has)
    mine = (r[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    win = key[pix[idx]] == mine
    cls[idx[~win]] = SHADOWED
    w = idx[win]
    pw = pix[w]
    cls[w] = np.where(ground[pw], GROUND, np.where(valid[np.maximum(lab[pw], 0)], SEGMENT, OUTLIER))
    seg[w] = np.where(ground[pw], -1, lab[pw])
    masked = pts.copy()
    drop = ((cfg.keep_classes >> cls.astype(np.int64)) & 1) == 0
    masked[drop, :3] = np.nan
    info = np.zeros(10, np.int32)
    info[:5] = np.bincount(cls, minlength=5)
    info[5] = occupied.sum()
    info[6] = len(roots)
    info[7] = valid[roots].sum()
    info[8] = n - drop.sum()
    return dict(cls=cls, segment=seg, masked=masked, info=info)


def segment_scans(pts, ring, off, cfg, tab=None, method="union"):
    """The batch: every scan on its own, the outputs back to back; info (n_scans, 10)."""
    tab = tables(cfg) if tab is None else tab
    pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 4))
    ring = np.asarray(ring)
    out = [segment_scan(pts[off[b]:off[b + 1]], ring[off[b]:off[b + 1]], cfg, tab, method) for b in range(len(off) - 1)]
    return dict(cls=np.concatenate([o["cls"] for o in out] + [np.zeros(0, np.uint8)]),
                segment=np.concatenate([o["segment"] for o in out] + [np.zeros(0, np.int32)]),
                masked=np.concatenate([o["masked"] for o in out] + [np.zeros((0, 4), F)]),
                info=np.stack([o["info"] for o in out]) if out else np.zeros((0, 10), np.int32))


def same_bits(a, b):
    """array_equal on the bit patterns (NaN equals NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
