"""Stage A (feature extraction) at its structural limits: the case table.

Every case is one or more clouds (pts, ring) in driver order, the status the extraction must report for each, and the figures
that put the case on its edge (`claim`).  tests/test_extract_limit_cases_model.py proves the figures on the CPU, with the oracle and
plain arithmetic; tests/test_gpu_extract_limits.py runs the kernels on the cases, on every ring-split form.  All cases use the
default parameters (six sectors, 2 / 20 / 4 picks, thresholds 0.1 and 0.05).

Coordinates are multiples of 2^-4 below 2^10 in magnitude: an 11-tap curvature sum then needs at most 19 bits, every f32 sum is
exact whatever its order, and identical local shapes give identical curvature bits (ties on purpose, not by luck).

Two geometries:
  sweep   x = 8, y falling by 1/8 per point of the driver-order cloud and passing y = 0, the direction of the cloud's first point,
          between the points w - 1 and w: the relative angle rises towards 2 pi and drops at w, so every ring takes the +2 pi
          time from its first point at or behind w that has a predecessor on its ring.  z carries the ring and a bump every few
          points (curvature without touching the azimuth).
  line    one ring along y with step 1/4 (squared gap 0.0625 > 0.05: a pick suppresses only itself) or 1/8 (0.0156: neighbour
          suppression on), x = 8 plus bumps: + 1/2 ("big": curvature 25 at the bump, 0.25 at the ten points around it, squared gap
          beside it 0.27) or + 1/16 ("small": curvature 0.39 at the bump, 0.0039 around it, squared gap 0.0195: a corner whose
          suppression window is the full eleven points).

Groups (docs/kernels/extraction.md, "Structural limits"):
  slices_*    1  cloud sizes around the 64-point group, the 256-point pre-pass and iteration, the slice lengths of every G
  rings_*     2  ring-id sets: {0}, {127}, {0, 64, 127}, the seven one-bit ids inside one group, all 128
  head_*      3  the first valid point behind 4 001 invalid ones
  badring_*   4  a ring id >= 128 on the last point; on invalid points only
  wrap_*      5  planted wraps, one per predecessor path of the +2 pi test
  ringlen_*, ends_*   6  ring lengths 1..24, 10 / 11 / 16 / 17, sector sizes 64 / 512 / 513, corners at a ring's first and last
              pickable position (also on four rings side by side, at the ring capacity)
  tie_*, flat_*       7  equal curvature bits inside a lane and across lanes, corner and flat pass, LDS and re-read path
  seam_*      8  picks on either side of a sector seam, suppression windows that start at bit 27..31 of a mask word
  tiles_*     9  n_full within +-6 of a curvature tile edge, 300 invalid points per scan
  compact_*   10 less-flat totals of 4 095 / 4 096 / 4 097 and 65 535 / 65 536 / 65 537
  batch_*     11 refused scans between good ones; B on either side of every threshold of G
"""
import functools
from dataclasses import dataclass, field

import numpy as np

OK, BAD_ARG, BAD_RING, CAPACITY = 0, 3, 5, 7
SCAN_PERIOD = 0.1
PICK_SECTOR = 512                      # kPickSector: the largest sector picked from LDS candidates
RING_CAPACITY = 8128
SPLITS = (1, 2, 4, 8, 16)              # MSFL_PREP_SPLIT
Y_LIMIT = 1000.0 + 2.0 ** -4           # sweeps longer than 16 000 points stand still beyond it (equal angles never wrap)


@dataclass
class Case:
    name: str
    clouds: list                        # [(pts (n, 4) float32, ring (n,) uint16), ...] in driver order
    status: list                        # the msfl_status of each cloud
    claim: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------------------------- arithmetic of the kernels
def sector_bounds(length):
    """Ring-local [sp, ep] of the six sectors of a ring of `length` points; [] when the ring is too short to be picked."""
    start, end = 5, length - 6
    if end - start < 6:
        return []
    return [(start + (end - start) * j // 6, start + (end - start) * (j + 1) // 6 - 1) for j in range(6)]


def sector_sizes(length):
    return [ep - sp + 1 for sp, ep in sector_bounds(length)]


def sector_of(length, pos):
    for j, (sp, ep) in enumerate(sector_bounds(length)):
        if sp <= pos <= ep:
            return j
    return None


def slice_len(n, G):
    """Points per slice of the ring split with G workgroups per scan (16 G slices, multiples of 64)."""
    S = 16 * G
    return ((n + S - 1) // S + 63) & ~63


def slice_populations(n, G):
    sl = slice_len(n, G)
    return [max(0, min(n, (k + 1) * sl) - min(n, k * sl)) for k in range(16 * G)]


def wrap_path(ring, w, G):
    """Which predecessor the wrap test of point w (all points valid) compares with on the G-workgroup form:
    1 the previous same-ring lane of its 64-point group, 2 the wavefront's last point of the ring, 3 the same across the
    256-point boundary of the four-groups-per-iteration loop, 4 the last point of the slice before it (same workgroup),
    5 the same in an earlier workgroup, 6 a slice further back, the slices in between holding none of the ring; 0 none."""
    prev = np.flatnonzero(ring[:w] == ring[w])
    if len(prev) == 0:
        return 0
    p, sl = int(prev[-1]), slice_len(len(ring), G)
    if p // 64 == w // 64:
        return 1
    if p // sl == w // sl:
        return 2 if (p % sl) // 256 == (w % sl) // 256 else 3
    if w // sl - p // sl > 1:
        return 6
    return 4 if (p // sl) // 16 == (w // sl) // 16 else 5


def expected_wraps(ring, w):
    """ring id -> cloud index of the ring's wrap point in a sweep that passes the start direction between w - 1 and w: the ring's
    first point at or behind w, if the ring has a point in front of w other than the cloud's first (whose relative angle is 0:
    nothing can fall below it, which is also why no wrap can sit at cloud index 1).  None: the ring never wraps."""
    out = {}
    for r in np.unique(ring):
        k = np.flatnonzero(ring == r)
        behind = k[k >= w] if w is not None else k[:0]
        wraps = len(behind) > 0 and behind[0] > k[0] and k[k < behind[0]][-1] != 0
        out[int(r)] = int(behind[0]) if wraps else None
    return out


# ---------------------------------------------------------------------------------------------- building blocks
def _cloud(x, y, z):
    p = np.zeros((len(x), 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = x, y, z
    return p


def sweep(ring, w, bump=7):
    """The sweep geometry over the ring sequence `ring`; w = None: y stays positive (no wrap)."""
    ring = np.asarray(ring, np.uint16)
    n = len(ring)
    k = np.arange(n)
    y = ((n if w is None else w) - k) * 0.125 - 0.0625
    y = np.clip(y, -Y_LIMIT, Y_LIMIT)
    if n:
        y[0] = 0.0
    slot = np.searchsorted(np.unique(ring), ring)
    z = 0.25 * (slot % 64) + (0.5 * (k % bump == 0) if bump else 0.0)
    return _cloud(np.full(n, 8.0), y, z), ring


def cycle(n, ids):
    return np.asarray(ids, np.uint16)[np.arange(n) % len(ids)]


def line(n, step, big=(), small=(), ring_id=0, z=0.0):
    """The line geometry: one ring of n points."""
    x = np.full(n, 8.0)
    x[np.asarray(list(big), np.int64)] += 0.5
    x[np.asarray(list(small), np.int64)] += 0.0625
    y = (np.arange(n) - n // 2) * step
    return _cloud(x, y, np.full(n, z)), np.full(n, ring_id, np.uint16)


def sawtooth(n, P, step):
    return line(n, step, big=range(0, n, P))


def interleave(rings):
    """Per-ring clouds [(pts, ring)] -> one driver-order cloud, round robin over the rings that still have points."""
    i = np.concatenate([np.arange(len(p)) for p, _ in rings])
    j = np.concatenate([np.full(len(p), k) for k, (p, _) in enumerate(rings)])
    order = np.lexsort((j, i))
    return np.concatenate([p for p, _ in rings])[order], np.concatenate([r for _, r in rings])[order]


def with_invalid(pts, ring, n_front, n_mid, n_back):
    """Invalid points around a cloud: NaN ones in front, too-near ones after its 50th point, infinite ones behind."""
    bad = lambda n, v: (np.tile(np.array(v, np.float32), (n, 1)), np.full(n, ring[0], np.uint16))
    parts = [bad(n_front, [np.nan, 1, 1, 0]), (pts[:50], ring[:50]), bad(n_mid, [0.0625, 0.125, 0, 0]), (pts[50:], ring[50:]),
             bad(n_back, [8, np.inf, 0, 0])]
    return np.concatenate([p for p, _ in parts]), np.concatenate([r for _, r in parts])


def _one(name, cloud, claim=None, status=OK):
    return Case(name, [cloud], [status], claim or {})


# ---------------------------------------------------------------------------------------------- 1: slices and groups
SLICE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16385)
SLICE_CLAIMS = {   # n -> {G: (non-empty slices, points in the last non-empty one)}
    65: {16: (2, 1)}, 257: {16: (5, 1), 1: (5, 1)}, 1023: {16: (16, 63), 1: (16, 63)}, 1025: {1: (9, 1), 16: (17, 1)},
    4097: {16: (65, 1), 1: (13, 257)}, 16385: {16: (129, 1), 1: (16, 65)},
}


def _slices(name):
    n = int(name.split("_")[1])
    c = sweep(cycle(n, (0, 3, 5, 10, 15)), 2 * n // 3 if n > 1 else None)
    return _one(name, c, dict(n=n, slices=SLICE_CLAIMS.get(n, {})))


# ---------------------------------------------------------------------------------------------- 2: ring id sets
RING_SETS = {"rings_0": (200, (0,)), "rings_127": (200, (127,)), "rings_0_64_127": (300, (0, 64, 127)),
             "rings_one_bit": (140, (1, 2, 4, 8, 16, 32, 64)), "rings_all_128": (2560, tuple(range(128)))}


def _rings(name):
    n, ids = RING_SETS[name]
    return _one(name, sweep(cycle(n, ids), n // 2), dict(ids=ids))


# ---------------------------------------------------------------------------------------------- 3, 4: invalid heads, bad ring ids
def _head(name):
    p, r = sweep(cycle(699, (1, 6, 11)), 400)
    junk = np.zeros((4001, 4), np.float32)
    junk[0::2, 0] = np.nan
    junk[1::2, :3] = [0.125, 0.0625, 0.0]                     # norm 0.14: inside the minimum range
    return _one(name, (np.concatenate([junk, p]), np.concatenate([cycle(4001, (1, 6, 11)), r])), dict(first_valid=4001, n_full=699))


def _badring(name):
    if name == "badring_last_point":
        p, r = sweep(cycle(5000, (0, 7, 9)), 3000)
        r[-1] = 128
        return _one(name, (p, r), status=BAD_RING)
    p, r = sweep(cycle(500, (0, 7, 9)), 300)
    p[100, 0] = np.nan; r[100] = 300
    p[200, :3] = [0.125, 0.0625, 0.0]; r[200] = 128
    return _one(name, (p, r), dict(n_full=498))


# ---------------------------------------------------------------------------------------------- 5: planted wraps
WRAP_N = 4100                       # slices of 320 points at G = 1, of 64 at G = 16 (workgroups of 1 024)
WRAP_IDS = (2, 9, 77)
WRAP_W = {   # name -> (w, {G: predecessor path})
    "wrap_2": (2, {1: 1, 16: 1}), "wrap_63": (63, {1: 1, 16: 1}), "wrap_64": (64, {1: 2, 16: 4}), "wrap_65": (65, {1: 2, 16: 4}),
    "wrap_255": (255, {1: 1, 16: 1}), "wrap_256": (256, {1: 3, 16: 4}), "wrap_257": (257, {1: 3, 16: 4}),
    "wrap_319": (319, {1: 1, 16: 1}), "wrap_320": (320, {1: 4, 16: 4}),
    "wrap_1023": (1023, {1: 1, 16: 1}), "wrap_1024": (1024, {1: 2, 16: 5}),
    "wrap_last": (WRAP_N - 1, {1: 1, 16: 1}), "wrap_none": (None, {}),
}
WRAP_OTHER = ("wrap_big_64", "wrap_grouped_256", "wrap_grouped_1280", "wrap_early_and_late")


def _wrap(name):
    if name in WRAP_W:
        w, paths = WRAP_W[name]
        ring = cycle(WRAP_N, WRAP_IDS)
        if w == 2:
            ring[1] = ring[2]                                  # the earliest wrap there can be: point 1 in front of the start direction, point 2 behind it
    elif name == "wrap_big_64":                                # 16 385 points: slices of 128 at G = 16, so the predecessor is the wavefront's
        w, paths, ring = 64, {1: 2, 16: 2}, cycle(16385, WRAP_IDS)
    elif name == "wrap_grouped_256":                           # ring 2 in [0, 64), ring 9 in [64, 256), ring 2 again from 256 on
        w, paths = 256, {1: 3, 16: 6}
        ring = np.r_[np.full(64, 2), np.full(192, 9), np.full(WRAP_N - 256, 2)].astype(np.uint16)
    elif name == "wrap_grouped_1280":                          # ring 2 in [0, 320), ring 9 in [320, 1280), ring 2 again from 1280 on
        w, paths = 1280, {1: 6, 16: 6}
        ring = np.r_[np.full(320, 2), np.full(960, 9), np.full(WRAP_N - 1280, 2)].astype(np.uint16)
    else:                                                      # ring 2 wraps at 100 (pre-pass), ring 9 at 1000 (late fix-up), ring 77 never
        w, paths = 100, {1: 1, 16: 1}
        ring = np.r_[cycle(100, (2, 9)), cycle(900, (2, 77)), np.full(3100, 0)].astype(np.uint16)
        ring[1000:] = np.asarray((2, 9, 77), np.uint16)[np.arange(1000, WRAP_N) % 3]
    claim = dict(w=w, paths=paths, wraps=expected_wraps(ring, w))
    return _one(name, sweep(ring, w, bump=0), claim)


# ---------------------------------------------------------------------------------------------- 6: ring lengths
def _ringlen(name):
    if name == "ringlen_1_to_24":
        rings = [_cloud(8.0 + 0.5 * (np.arange(r + 1) % 5 == 2), (np.arange(r + 1) - 12) * 0.25, np.full(r + 1, 0.25 * r)) for r in range(24)]
        return _one(name, interleave([(p, np.full(len(p), r, np.uint16)) for r, p in enumerate(rings)]), dict(lengths=list(range(1, 25))))
    n = int(name.split("_")[1])
    return _one(name, line(n, 0.25, big=[n // 2]), dict(lengths=[n], sizes=sector_sizes(n)))


def ends_ring(n, ring_id=0):
    return line(n, 0.125, small=[5, n - 7], ring_id=ring_id, z=0.25 * ring_id)


def _ends(name):
    n = int(name.split("_")[1])
    if name.endswith("_x4"):                                   # rings 4..7: the four wavefronts of one pick workgroup
        c = interleave([ends_ring(n, r) for r in (4, 5, 6, 7)])
        return _one(name, c, dict(lengths=[n] * 4, ring_ids=[4, 5, 6, 7], corners=[5, n - 7]))
    return _one(name, ends_ring(n), dict(lengths=[n], ring_ids=[0], corners=[5, n - 7], sizes=sector_sizes(n)))


# ---------------------------------------------------------------------------------------------- 7: ties
TIE_LENS = (395, 3083, 3084, 3700)


def tie_pairs(n, positions):
    """(a, b, lanes) for the two highest of `positions` in every sector that holds two: lanes = 'same' / 'cross'."""
    out = []
    for sp, ep in sector_bounds(n):
        inside = [q for q in positions if sp <= q <= ep]
        if len(inside) >= 2:
            a, b = inside[-1], inside[-2]
            out.append((a, b, "same" if (a - sp) % 64 == (b - sp) % 64 else "cross"))
    return out


def _tie(name):
    _, n, P, step = name.split("_")                            # tie_3083_64_s4: step 1/4 (s4) or 1/8 (s8)
    n, P, step = int(n), int(P), {"s4": 0.25, "s8": 0.125}[step]
    return _one(name, sawtooth(n, P, step), dict(lengths=[n], sizes=sector_sizes(n), sharp_pairs=tie_pairs(n, list(range(0, n, P))), step=step))


def inlane_flat_positions(n, c=40):
    return [f for f in range(c, n, 64) if 5 <= f <= n - 7]


def inlane_flat_ring(n, c=40):
    """Big bumps such that every point but those at c + 64 m has one within five points: the only flat candidates are 64 apart."""
    bumps = set(range(c - 6, -1, -10))
    for f in range(c, n + 64, 64):
        bumps |= {f + 6 + 10 * j for j in range(6)} | {f + 58}
    return line(n, 0.25, big=sorted(b for b in bumps if 0 <= b < n))


def _flat(name):
    kind, n = name.split("_")[1], int(name.split("_")[2])
    if kind == "inlane":                                       # the four lowest candidates of a sector, all in one lane
        pos = inlane_flat_positions(n)
        pairs = []
        for sp, ep in sector_bounds(n):
            inside = [q for q in pos if sp <= q <= ep]
            pairs += [(a, b, "same") for a, b in zip(inside[:3], inside[1:4])]
        return _one(name, inlane_flat_ring(n), dict(lengths=[n], sizes=sector_sizes(n), flat_pairs=pairs))
    # a sawtooth of period 64: the zero-curvature points are runs of 53, so a sector's four flat picks sit in neighbouring lanes
    far = [q for q in range(n) if min(q % 64, 64 - q % 64) > 5]
    pairs = []
    for sp, ep in sector_bounds(n):
        inside = [q for q in far if sp <= q <= ep]
        pairs += [(a, b, "cross") for a, b in zip(inside[:3], inside[1:4])]
    return _one(name, sawtooth(n, 64, 0.25), dict(lengths=[n], sizes=sector_sizes(n), flat_pairs=pairs))


# ---------------------------------------------------------------------------------------------- 8: sector seams
def _seam(name):
    _, kind, n = name.split("_")
    n = int(n)
    sec = sector_bounds(n)
    if kind == "bits":                                          # suppression windows [q - 5, q + 5] that start at bit 27..31 of a mask word
        corners = [96, 161, 226, 291, 356]
        return _one(name, line(n, 0.125, small=corners), dict(lengths=[n], corners=corners, window_bits=[(q - 5) & 31 for q in corners]))
    j = 4 if n == 3084 else 2                                  # len 3 084: sector 4 is picked from LDS, sector 5 (513 points) by re-reading;
                                                               # len 3 085 (512, 512, 513, 512, 512, 513): sector 2 by re-reading, sector 3 from LDS
    if kind == "last":
        # a corner at sector j's last position kills the five points behind the seam; big bumps make every other point of sector
        # j + 1 a corner, so sector j + 1 has no flat candidate left
        q = sec[j][1]
        big = [b for b in range(q + 11, sec[j + 1][1] + 11, 10) if b < n]
        return _one(name, line(n, 0.125, big=big, small=[q]),
                    dict(lengths=[n], sizes=sector_sizes(n), corners=[q], label2=list(range(q + 1, q + 6)), no_flat_in=sec[j + 1]))
    # a corner at sector j + 1's first position relabels the last five points of sector j, whose less-flat list is out already
    q = sec[j + 1][0]
    return _one(name, line(n, 0.125, small=[q]),
                dict(lengths=[n], sizes=sector_sizes(n), corners=[q], label2=list(range(q - 5, q)), less_flat_has=list(range(q - 5, q))))


# ---------------------------------------------------------------------------------------------- 9: curvature tiles
TILE_NFULL = tuple(range(250, 263)) + tuple(range(506, 519))


def _tiles(name):
    clouds = [with_invalid(*sawtooth(nf, 16, 0.25), 100, 100, 100) for nf in TILE_NFULL]
    return Case(name, clouds, [OK] * len(clouds), dict(n_full=list(TILE_NFULL), raw=[nf + 300 for nf in TILE_NFULL]))


# ---------------------------------------------------------------------------------------------- 10: compact pieces
COMPACT = {"compact_4095": [1376, 1376, 1376], "compact_4096": [1376, 1376, 1377], "compact_4097": [1376, 1377, 1377],
           "compact_65535": [4107] * 15 + [4106], "compact_65536": [4107] * 16, "compact_65537": [4107] * 15 + [4108]}


def _compact(name):
    lens = COMPACT[name]
    c = interleave([line(n, 0.25, ring_id=r, z=0.25 * r) for r, n in enumerate(lens)])
    return _one(name, c, dict(lengths=lens, less_flat=int(name.split("_")[1])))


# ---------------------------------------------------------------------------------------------- 11: batches
B_EDGES = (16, 17, 32, 33, 64, 65, 128, 129)
G_OF_B = {16: 16, 17: 8, 32: 8, 33: 4, 64: 4, 65: 2, 128: 2, 129: 1}


@functools.lru_cache(maxsize=None)
def tiny_pool():
    """Scans of 40 to 300 points: what the batches around the thresholds of G are made of."""
    pool = [sweep(cycle(n, ids), w) for n, ids, w in ((40, (0, 1), 20), (63, (3,), 40), (64, (0, 5, 9), 33), (65, (2, 4), 64), (100, (0, 127), 1),
                                                      (129, (7,), 128), (200, (1, 2, 3, 4), None), (255, (0, 15), 130), (256, (6, 8), 255),
                                                      (257, (0, 1, 2), 256), (300, (11,), 150))]
    pool += [case("ringlen_1_to_24").clouds[0], sawtooth(300, 16, 0.125), case("rings_one_bit").clouds[0]]
    return pool


def batch_of(B):
    pool = tiny_pool()
    return [pool[(b + B) % len(pool)] for b in range(B)]


def _batch(name):
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.uint16))
    nanc = sweep(cycle(200, (0, 1)), 100)
    nanc[0][:, 1] = np.nan
    badr = sweep(cycle(200, (0, 1)), 100)
    badr[1][50] = 200
    clouds = [sweep(cycle(300, (0, 4, 8)), 150), empty, nanc, badr, line(RING_CAPACITY + 1, 0.125), sawtooth(395, 16, 0.25)]
    # the oracle has no ring capacity: it extracts the 8 129-point ring; every other status is the oracle's
    return Case(name, clouds, [OK, BAD_ARG, BAD_ARG, BAD_RING, CAPACITY, OK], dict(oracle_status=[0, 3, 3, 5, 0, 0]))


# ---------------------------------------------------------------------------------------------- the table
_FAMILIES = {"slices": _slices, "rings": _rings, "head": _head, "badring": _badring, "wrap": _wrap, "ringlen": _ringlen, "ends": _ends,
             "tie": _tie, "flat": _flat, "seam": _seam, "tiles": _tiles, "compact": _compact, "batch": _batch}

NAMES = (["slices_%d" % n for n in SLICE_SIZES]
         + list(RING_SETS)
         + ["head_4001_invalid", "badring_last_point", "badring_on_invalid_only"]
         + list(WRAP_W) + list(WRAP_OTHER)
         + ["ringlen_1_to_24", "ringlen_10", "ringlen_11", "ringlen_16", "ringlen_17", "ends_395", "ends_8128", "ends_8128_x4"]
         + ["tie_%d_%d_%s" % (n, P, s) for n in TIE_LENS for P in (7, 16, 64) for s in ("s4", "s8")] + ["tie_800_16_s8", "tie_3088_7_s4"]
         + ["flat_inlane_3083", "flat_inlane_3700", "flat_cross_3083", "flat_cross_3700"]
         + ["seam_last_800", "seam_last_3084", "seam_last_3085", "seam_last_3700", "seam_first_800", "seam_first_3084", "seam_first_3085",
            "seam_first_3700", "seam_bits_800"]
         + ["tiles_26_scans"]
         + list(COMPACT))
REFUSED_BATCH = "batch_refused_between_good"
SANDWICH = ("slices_257", "ringlen_17")      # the clouds a case stands between when it runs inside a batch


@functools.lru_cache(maxsize=None)
def case(name):
    return _FAMILIES[name.split("_")[0]](name)
