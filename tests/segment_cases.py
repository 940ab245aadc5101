"""Scenes for the segmentation tests (tests/test_segment_model.py on the CPU, tests/test_gpu_segment.py on the GPU): hand scenes
with hand-written expected classes on 8 x 64 images, component shapes where a union-find can go wrong on 16 x 64 images, seeded
random images and real sweeps of the synthetic worlds.  A scene is (name, pts, ring, cfg[, expected classes])."""
import numpy as np

import segment_numpy as sn

N, S, G, SEG, O = sn.NONE, sn.SHADOWED, sn.GROUND, sn.SEGMENT, sn.OUTLIER


def hand_config(**kw):
    """8 x 64 pixels, -15 .. +15 degrees (rows 0..3 look down), three ground row pairs, the default thresholds."""
    return sn.config(**{**dict(n_col=64, n_row=8, ground_rows=3), **kw})


def stress_config(**kw):
    return sn.config(**{**dict(n_col=64, n_row=16, ground_rows=0, elev_low_deg=-15.0, elev_high_deg=15.0), **kw})


def beam(cfg, row, col, r, daz=0.0):
    """The point at range r on the beam through the centre of pixel (row, col) (daz: azimuth offset in columns)."""
    az = 2.0 * np.pi * (col + daz) / cfg.n_col
    el = np.deg2rad(sn.elevations_deg(cfg)[row])
    return [r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), 0.0]


class Scene:
    def __init__(self, cfg):
        self.cfg, self.pts, self.ring, self.want = cfg, [], [], []

    def put(self, row, col, r, want, daz=0.0):
        self.pts.append(beam(self.cfg, row, col, r, daz))
        self.ring.append(row)
        self.want.append(want)

    def raw(self, xyz, ring, want):
        self.pts.append(list(xyz) + [0.0])
        self.ring.append(ring)
        self.want.append(want)

    def done(self, name):
        return name, np.asarray(self.pts, np.float32).reshape(-1, 4), np.asarray(self.ring, np.uint16), self.cfg, np.asarray(self.want, np.uint8)


def _ground_range(cfg, row, height=1.8):
    return height / -np.sin(np.deg2rad(sn.elevations_deg(cfg)[row]))


def _slope_pair(cfg, theta_deg, r0=5.0):
    """Ranges of two points in rows 0 and 1 of one column whose difference rises at theta above the horizontal."""
    e = np.deg2rad(sn.elevations_deg(cfg))
    t = np.tan(np.deg2rad(theta_deg))
    return r0, r0 * (np.sin(e[0]) - t * np.cos(e[0])) / (np.sin(e[1]) - t * np.cos(e[1]))


def hand_scenes():
    out = []
    cfg = hand_config()
    s = Scene(cfg)                                                # level ground: rows 0..3 of every column, the sensor 1.8 m up
    for col in range(64):
        for row in range(4):
            s.put(row, col, _ground_range(cfg, row), G)
    out.append(s.done("level_ground"))
    for name, theta, want in (("slope_inside", 9.5, G), ("slope_outside", 10.5, O)):
        s = Scene(cfg)                                            # ground angle 10 degrees; outside it: a component of two pixels
        r0, r1 = _slope_pair(cfg, theta)
        s.put(0, 7, r0, want)
        s.put(1, 7, r1, want)
        out.append(s.done(name))
    s = Scene(cfg)                                                # a box: 4 rows x 10 columns at 10 m
    for row in range(4, 8):
        for col in range(10, 20):
            s.put(row, col, 10.0, SEG)
    out.append(s.done("box"))
    s = Scene(cfg)                                                # two boxes a range jump apart: 10 m and 20 m in neighbouring columns
    for row in range(4, 8):
        for col in range(10, 22):
            s.put(row, col, 10.0 if col < 16 else 20.0, SEG)
    out.append(s.done("two_boxes"))
    for name, n, want in (("blob_29", 29, O), ("blob_30", 30, SEG)):
        s = Scene(cfg)                                            # two rows: 15 pixels and the rest
        for k in range(n):
            s.put(4 + k // 15, 20 + k % 15, 8.0, want)
        out.append(s.done(name))
    s = Scene(cfg)                                                # 5 pixels over 3 rows: the tall rule
    for row, col in ((4, 30), (5, 30), (6, 30), (4, 31), (5, 31)):
        s.put(row, col, 6.0, SEG)
    out.append(s.done("pole_3_rows"))
    s = Scene(cfg)                                                # 5 pixels over 2 rows: too flat for it
    for row, col in ((4, 30), (5, 30), (4, 31), (5, 31), (4, 32)):
        s.put(row, col, 6.0, O)
    out.append(s.done("pole_2_rows"))
    s = Scene(cfg)                                                # across the turn: columns 62, 63, 0, 1
    for row in range(4, 7):
        for col in (62, 63, 0, 1):
            s.put(row, col, 12.0, SEG)
    out.append(s.done("wrap"))
    s = Scene(cfg)                                                # two points in one pixel: the nearer wins; equal range: the lower index
    s.put(5, 40, 12.0, S)
    s.put(5, 40, 10.0, O)
    s.put(6, 41, 9.0, O)
    s.put(6, 41, 9.0, S)
    out.append(s.done("shadowed"))
    s = Scene(cfg)
    s.raw((np.nan, 1.0, 1.0), 3, N)
    s.raw((1.0, np.inf, 1.0), 3, N)
    s.raw((0.0, 0.0, 5.0), 3, N)                                  # on the axis
    s.put(5, 3, 200.0, N)                                         # beyond max_range
    s.put(5, 4, 0.1, N)                                           # inside min_range
    s.raw(beam(cfg, 5, 5, 7.0)[:3], 8, N)                         # ring n_row
    s.put(5, 6, 7.0, O)                                           # and one that counts
    out.append(s.done("no_pixel"))
    return out


def _mask_scene(name, mask, cfg, r=10.0):
    s = Scene(cfg)
    for row, col in zip(*np.nonzero(mask)):
        s.put(int(row), int(col), r, SEG)
    return s.done(name)


def _spiral(r0, r1, c0, c1, pitch=4):
    """Pixels of a rectangular spiral winding inwards from (r0, c0), its arms `pitch` apart."""
    px, r, c = [], r0, c0
    top, bot, left, right = r0 + pitch, r1, c0, c1
    while True:
        if right <= c: break
        px += [(r, k) for k in range(c, right + 1)]; c = right; right -= pitch
        if bot <= r: break
        px += [(k, c) for k in range(r, bot + 1)]; r = bot; bot -= pitch
        if left >= c: break
        px += [(r, k) for k in range(c, left - 1, -1)]; c = left; left += pitch
        if top >= r: break
        px += [(k, c) for k in range(r, top - 1, -1)]; r = top; top += pitch
    return px


def stress_scenes():
    """(name, pts, ring, cfg, want, n_components) on 16 x 64 images, every occupied pixel at 10 m."""
    cfg = stress_config()
    out = []
    m = np.zeros((16, 64), bool)                                  # serpentine: full rows with a gap at column 31, joined at alternating sides of it
    for row in range(16):
        if row % 2 == 0:
            m[row] = True
            m[row, 31] = False
        else:
            m[row, 30 if row % 4 == 1 else 32] = True
    out.append(_mask_scene("serpentine", m, cfg) + (1,))
    m = np.zeros((16, 64), bool)                                  # comb: teeth in the even columns, joined only in the last row
    m[:15, 0::2] = True
    m[15] = True
    out.append(_mask_scene("comb", m, cfg) + (1,))
    m = np.zeros((16, 64), bool)                                  # a ring round the whole turn
    m[8] = True
    out.append(_mask_scene("ring", m, cfg) + (1,))
    m = np.zeros((16, 64), bool)                                  # two interleaved spirals that never touch
    # the second one runs down the middle of the first one's gaps (its innermost arm, row 7, would touch the first one's row 8)
    for r, c in _spiral(0, 13, 1, 58) + [p for p in _spiral(2, 11, 3, 56) if not (p[0] == 7 and 7 <= p[1] <= 52)]:
        m[r, c] = True
    out.append(_mask_scene("spirals", m, cfg) + (2,))
    return out


def random_image(seed, n_row, n_col, fill=0.8, extra=0.15, **kw):
    """A seeded image: ranges from a few depth layers in blocks plus noise, random holes, `extra` second points in random pixels
    (some at the very range of the first), a handful of points without a pixel; the points in random order."""
    rng = np.random.default_rng(seed)
    cfg = sn.config(**{**dict(n_col=n_col, n_row=n_row, ground_rows=min(n_row - 1, max(n_row // 2, 1)), elev_low_deg=-15.0, elev_high_deg=15.0), **kw})
    layers = np.array([4.0, 9.0, 9.6, 25.0, 60.0])
    br, bc = max(n_row // 4, 1), max(n_col // 16, 1)
    blocks = rng.integers(0, len(layers), (n_row // br + 1, n_col // bc + 1))
    row, col = np.meshgrid(np.arange(n_row), np.arange(n_col), indexing="ij")
    r = layers[blocks[row // br, col // bc]] + rng.normal(0, 0.05, (n_row, n_col))
    low = np.deg2rad(sn.elevations_deg(cfg))[row] < -0.02
    flat = low & (rng.random((n_row, n_col)) < 0.5)                # half of the downward beams see level ground
    r = np.where(flat, 1.8 / -np.sin(np.minimum(np.deg2rad(sn.elevations_deg(cfg))[row], -0.02)), r)
    keep = rng.random((n_row, n_col)) < fill
    row, col, r = row[keep], col[keep], r[keep]
    k = rng.integers(0, len(row), int(extra * len(row)))          # second points
    r2 = np.where(rng.random(len(k)) < 0.3, r[k], r[k] + rng.uniform(-1.0, 1.0, len(k)))
    row, col, r = np.concatenate([row, row[k]]), np.concatenate([col, col[k]]), np.concatenate([r, r2])
    daz = np.concatenate([rng.uniform(-0.4, 0.4, len(row) - len(k)), np.zeros(len(k))])
    daz[len(daz) - len(k):] = daz[k] * (rng.random(len(k)) < 0.5)
    az = 2.0 * np.pi * (col + daz) / n_col
    el = np.deg2rad(sn.elevations_deg(cfg))[row]
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.random(len(r))], axis=1).astype(np.float32)
    ring = row.astype(np.uint16)
    junk = np.array([[np.nan, 1, 1, 0], [0, 0, 3, 0], [500, 0, 0, 0], [0.01, 0.01, 0, 0], [1, 1, -np.inf, 0]], np.float32)
    pts, ring = np.concatenate([pts, junk]), np.concatenate([ring, np.array([0, 1, 0, 1, 0], np.uint16)])
    pts = np.concatenate([pts, pts[:2]]); ring = np.concatenate([ring, np.array([n_row, 200], np.uint16)])      # rings outside the image
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(ring[order]), cfg


def ragged_batch(seed=11, n_scans=37):
    """37 scans of a 6 x 32 image, an empty scan and a one-point scan among them: (pts, ring, off, cfg)."""
    pts, ring, off, cfg = [], [], [0], None
    for b in range(n_scans):
        p, r, cfg = random_image(seed + b, 6, 32, fill=0.3 + 0.6 * ((b * 7) % 10) / 10.0, min_points=6, min_points_tall=3, min_rows_tall=2)
        if b == 5:
            p, r = p[:0], r[:0]
        if b == 17:
            p, r = p[:1], r[:1]
        pts.append(p); ring.append(r); off.append(off[-1] + len(p))
    return np.concatenate(pts), np.concatenate(ring), np.asarray(off, np.int32), cfg


def sweep(kind, seed_offset=0, with_kind=False):
    """One sweep of the room or the outdoor world from one of the world's own poses."""
    from msf_loam_amd import synth
    world = synth.World(kind=kind) if kind != "room" else synth.World(ground_half=45.0)
    pose = synth.world_poses(world, 3)[seed_offset % 3]
    return synth.make_scan(world, pose, synth.SEED + 40 + seed_offset, with_kind=with_kind)
