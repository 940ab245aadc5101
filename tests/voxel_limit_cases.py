"""The voxel filter at its structural limits: the case table.

Every case is a batch of clouds and a power-of-two leaf (inv_leaf and the voxel boundaries are exact in f32), seeded by its name.
Points stand at (cell + u) * leaf with u in [0.05, 0.95] and carry a random 4th field, so the voxel of every point is known by
construction and the order in which a voxel's points are summed changes the f32 bits of its centroid.  A case names the form of
the filter that has to deliver its target cloud and the hand-overs on the way there (`path`: (form, flag, reason) per form that
looks at the cloud, as tests/voxel_form_model.py computes them), plus the figures that put it on its edge (`claim`).
tests/test_voxel_form_model.py proves both for every case on the CPU; tests/test_gpu_voxel_limits.py runs the filter on them.

Families (docs/kernels/voxel.md, "Structural limits"):
  P  point counts           1, 63, 64, 65; 4 095 / 4 096 / 4 097 (S -> L); 65 535 / 65 536 (L -> B); 131 071 / 131 072 (B -> G)
  R  run pools              2 048 / 2 049, 12 288 / 12 289, 65 536 / 65 537 runs
  C  coordinate fields      +-8 190 / +-8 191 (L), +-4 094 / +-4 095 (B), per axis and sign
  K  cell-index width       boxes of 8 / 9, 16 / 17, 24 / 25 and 31 index bits, pairs that differ only in the sort's last digit
  M  multi-run list         960 / 961 (S), 3 840 / 3 841 (L), 3 841 (B) voxels visited twice
  W  wavefront walk         a voxel with exactly 512 (thread) / 513 (wavefront) later points, in runs of 1, 2, 63, 64 and split ones,
                            drawn so that its forward, reversed and f64 sums differ in all four lanes
  Z  signed zeros           a lone -0.0 point, a two-run voxel whose sums cancel
  T  leaf too small         1290^3 cells accepted, 1291 x 1290 x 1290 refused in the middle of a batch
  X  coordinates no int holds   a finite coordinate beyond 1e9 and beyond 2^31 voxels
  Q  the device-wide key    65 536 / 65 537 clouds: 64 / 65 key bits (keys-only sort / (key, value) sort); at 65 also with a voxel
                            visited three times, whose runs only the sort's stability keeps in arrival order
"""
import functools
import itertools
import zlib
from dataclasses import dataclass, field

import numpy as np


@dataclass
class Case:
    name: str
    pts: np.ndarray                 # (n, 4) float32, the clouds back to back
    off: np.ndarray                 # (B + 1,) int32
    leaf: float
    target: int                     # the cloud the claim is about
    status: str                     # "OK" or "CAPACITY", on every handle
    path: list                      # default handle, target cloud: [(form, flag, reason), ...]
    voxels: object                  # voxels of the target cloud (None: refused)
    claim: dict = field(default_factory=dict)      # analysis / verdict figures that must hold exactly for the target
    scattered: bool = False         # delivered through idx / count from a scattered store

    @property
    def clouds(self):
        return [self.pts[self.off[b]:self.off[b + 1]] for b in range(len(self.off) - 1)]

    @property
    def form(self):
        """What delivers the target on the default handle: S, L, B, G or "refused"."""
        f, flag, _ = self.path[-1]
        return f if flag == 0 else "refused"


def serve_on(form, handle):
    """The serving form on the other handles, given the default handle's."""
    if form == "refused":
        return form
    if handle == "global":
        return "G"
    if handle == "no_big" and form == "B":
        return "G"
    return form


# ---------------------------------------------------------------------------------------------- building blocks
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def points_in(rng, cells, leaf):
    """One point per row of `cells` (n, 3), at (cell + u) * leaf, u in [0.05, 0.95]; random 4th field."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    c = np.zeros((len(cells), 4), np.float32)
    c[:, :3] = ((cells + rng.uniform(0.05, 0.95, cells.shape)) * leaf).astype(np.float32)
    c[:, 3] = rng.uniform(0.0, 1.0, len(cells))
    return c


def lattice(j, dims, origin):
    """Raster walk: lattice cell number j -> (x fastest) cell coordinates."""
    j = np.asarray(j, np.int64)
    assert j.size == 0 or int(j.max()) < dims[0] * dims[1] * dims[2]
    return np.stack([j % dims[0], (j // dims[0]) % dims[1], j // (dims[0] * dims[1])], axis=1) + np.asarray(origin, np.int64)


def sweep(n, per, dims, origin):
    """n points, `per` consecutive ones per voxel, never coming back: a slow sweep (n / per runs when per divides 64)."""
    return lattice(np.arange(n) // per, dims, origin)


def blocks(n_blocks, dims, origin):
    """Padding that adds nothing but points: 64-point blocks, each its own voxel.  Starting on a multiple of 64 every block is
    exactly one run, so the padding has no multi-run voxel and one run slot per 64 points."""
    return np.repeat(lattice(np.arange(n_blocks), dims, origin), 64, axis=0)


def _batch(clouds):
    off = np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(clouds), np.float32), off


def _single(name, cloud, leaf, path, voxels, claim=None, **kw):
    pts, off = _batch([cloud])
    return Case(name, pts, off, leaf, 0, "OK", path, voxels, claim or {}, **kw)


def seq_sum(p):
    """f32 sum of the rows of p in the order they stand, one addition after the other (what a thread of the filter does)."""
    return np.add.accumulate(np.asarray(p, np.float32), axis=0, dtype=np.float32)[-1]


def order_sensitive(p, others):
    """True when the points p, summed in their own order, differ in ALL FOUR lanes from each of `others` (f32 sums of the same
    points in another order, or their f64 sum rounded), as sums and as centroids."""
    n, s = np.float32(len(p)), seq_sum(p)
    return all(np.all(s.view(np.uint32) != o.view(np.uint32)) and np.all((s / n).view(np.uint32) != (o / n).view(np.uint32)) for o in others)


def redraw_until(rng, pts, cells, leaf, k, sensitive):
    """Redraw the points pts[k] (within their cells) until sensitive(pts[k]) holds: seeded, so the same draw every time."""
    for _ in range(10000):
        if sensitive(pts[k]):
            return
        pts[k] = points_in(rng, cells[k], leaf)
    raise AssertionError("no order-sensitive draw")


def _ordinary(rng, n, leaf):
    return points_in(rng, sweep(n, 4, (12, 12, 12), (-6, -6, -6)), leaf)


S_OK = [("S", 0, "served")]
L_BY_POINTS = [("S", 5, "points"), ("L", 0, "served")]
B_BY_POINTS = [("S", 5, "points"), ("L", 4, "points"), ("B", 0, "served")]
G_BY_POINTS = [("S", 5, "points"), ("L", 4, "points"), ("B", 4, "points"), ("G", 0, "served")]


def _path_for_size(size):
    return {"S": S_OK, "L": L_BY_POINTS, "B": B_BY_POINTS}[size]


# ---------------------------------------------------------------------------------------------- P: point counts
P_COUNTS = {1: S_OK, 63: S_OK, 64: S_OK, 65: S_OK, 4095: S_OK, 4096: S_OK, 4097: L_BY_POINTS, 65535: L_BY_POINTS, 65536: B_BY_POINTS,
            131071: B_BY_POINTS, 131072: G_BY_POINTS}


def _p(name, n):
    rng = _rng(name)
    cloud = points_in(rng, sweep(n, 8, (64, 64, 8), (-32, -32, -4)), 0.5)        # 8 points per voxel: n / 8 runs, inside every pool
    return _single(name, cloud, 0.5, P_COUNTS[n], (n + 7) // 8, dict(n=n, runs=(n + 7) // 8, multi=0))


# ---------------------------------------------------------------------------------------------- R: run pools
def _pairs_walk(n_runs, singles, dims, origin):
    """n_runs runs, every consecutive run in a new voxel: `singles` one-point runs, then two-point runs (on even positions when
    singles is even, so that no chunk boundary cuts one)."""
    assert singles % 2 == 0
    j = np.r_[np.arange(singles), singles + np.arange(2 * (n_runs - singles)) // 2]
    return lattice(j, dims, origin)


def _r(name):
    rng = _rng(name)
    spec = {
        "R_S_2048": (2048, 0, (13, 13, 13), S_OK),                                        # n = 4 096: both of S's limits at once
        "R_S_2049": (2049, 2, (13, 13, 13), [("S", 5, "runs"), ("L", 0, "served")]),      # n = 4 096 still: the escalation is the run pool's
        "R_L_12288": (12288, 0, (24, 24, 24), L_BY_POINTS),
        "R_L_12289": (12289, 2, (24, 24, 24), [("S", 5, "points"), ("L", 4, "runs"), ("B", 0, "served")]),
    }
    if name in spec:
        runs, singles, dims, path = spec[name]
        cells = _pairs_walk(runs, singles, dims, tuple(-(d // 2) for d in dims))
        return _single(name, points_in(rng, cells, 0.25), 0.25, path, runs, dict(runs=runs, n=len(cells), multi=0))
    n = {"R_B_65536": 65536, "R_G_65537": 65537}[name]                                   # all distinct on a 41^3 lattice walk
    path = B_BY_POINTS if n == 65536 else [("S", 5, "points"), ("L", 4, "points"), ("B", 4, "runs"), ("G", 0, "served")]
    cells = lattice(np.arange(n), (41, 41, 41), (-20, -20, -20))
    return _single(name, points_in(rng, cells, 0.25), 0.25, path, n, dict(runs=n, n=n, multi=0))


# ---------------------------------------------------------------------------------------------- C: coordinate fields
def _c(name):
    _, form, axis, sign, mag = name.split("_")                                            # C_L_x_neg_8191
    rng = _rng(name)
    mag, ax = int(mag), "xyz".index(axis)
    far = np.zeros((1, 3), np.int64)
    far[0, ax] = mag if sign == "pos" else -mag
    if form == "L":
        body = sweep(5000, 4, (20, 20, 20), (-10, -10, -10))                              # 5 001 points: S escalates on the count
        keeps = mag <= 8190
        path = L_BY_POINTS if keeps else [("S", 5, "points"), ("L", 4, "coordinates"), ("B", 4, "coordinates"), ("G", 0, "served")]
        nv = 1250 + 1
    else:
        body = sweep(65600, 8, (20, 21, 20), (-10, -10, -10))                             # > 65 535 points: L refuses on the count
        keeps = mag <= 4094
        path = B_BY_POINTS if keeps else [("S", 5, "points"), ("L", 4, "points"), ("B", 4, "coordinates"), ("G", 0, "served")]
        nv = 8200 + 1
    cells = np.concatenate([body[:2500], far, body[2500:]])
    return _single(name, points_in(rng, cells, 0.5), 0.5, path, nv, dict(coord_abs_max=float(mag)))


# ---------------------------------------------------------------------------------------------- K: cell-index width
K_BOXES = {"256x1x1": (8, 1), "257x1x1": (9, 2), "256x256x1": (16, 2), "257x256x1": (17, 3), "256x256x256": (24, 3),
           "257x256x256": (25, 4), "1290x1290x1290": (31, 4)}                             # box -> (nbits, radix passes)


def k_core_cells(rng, dims, passes, n_pairs=60, n_random=150):
    """Cell indices of a box's core points, in DESCENDING order: both corners (they fix the bounding box), pairs of cells whose
    indices differ only in the top radix digit, and random ones."""
    cells = dims[0] * dims[1] * dims[2]
    shift = 8 * (passes - 1)
    top = (cells - 1) >> shift
    picked = {0, cells - 1}
    if (top << shift) < cells:
        picked |= {0, top << shift}
    for _ in range(4000):
        if len(picked) >= 2 * n_pairs:
            break
        lo = int(rng.integers(0, 1 << shift)) if shift else 0
        t1, t2 = (int(t) for t in rng.integers(0, top + 1, 2))
        a, b = lo | (t1 << shift), lo | (t2 << shift)
        if t1 != t2 and a < cells and b < cells:
            picked |= {a, b}
    picked |= {int(c) for c in rng.integers(0, cells, n_random)}
    return np.array(sorted(picked, reverse=True), np.int64)


def _k(name):
    _, box, size = name.split("_")                                                        # K_257x256x1_L
    rng = _rng(name)
    dims = tuple(int(d) for d in box.split("x"))
    nbits, passes = K_BOXES[box]
    origin = tuple(-(d // 2) for d in dims)
    core = k_core_cells(rng, dims, passes)
    pad_row = np.arange(min(dims[0], 300))                                                # padding revisits the box's first row: the box stays what it is
    n_pad = {"S": 0, "L": 4100, "B": 65540}[size]
    per = -(-n_pad // len(pad_row)) if n_pad else 0
    pad = np.repeat(pad_row, per)[:n_pad] if n_pad else np.zeros(0, np.int64)
    idx = np.r_[pad, core]
    nv = len(set(idx.tolist()))
    return _single(name, points_in(rng, lattice(idx, dims, origin), 0.25), 0.25, _path_for_size(size), nv,
                   dict(nbits=nbits, radix_passes=passes, cells=dims[0] * dims[1] * dims[2]))


# ---------------------------------------------------------------------------------------------- M: multi-run list
def _m(name):
    _, form, count = name.split("_")
    N = int(count)
    rng = _rng(name)
    dims = (10, 10, 10) if form == "S" else (16, 16, 16)
    once = lattice(np.arange(N), dims, tuple(-(d // 2) for d in dims))
    cells = np.concatenate([once, once])                                                  # N voxels, one point each, then the same again
    nv = N
    if form == "B":
        pad = blocks(904, (32, 32, 1), (-16, -16, 12))                                    # 57 856 points in front, one run and one voxel per block
        cells = np.concatenate([pad, cells]); nv += 904
    cap = 960 if form == "S" else 3840
    return _single(name, points_in(rng, cells, 0.25), 0.25, _path_for_size(form), nv,
                   dict(multi=N, multi_overflow=max(N - cap, 0), later_max=1, n_big=0))


# ---------------------------------------------------------------------------------------------- W: wavefront walk
W_SPEC = {   # name -> (form, later points, voxels of that kind, points in all, 64-point padding blocks in front, scattered)
    "W_S_512": ("S", 512, 1, 2000, 0, False), "W_S_513": ("S", 513, 1, 2000, 0, False), "W_S_513_idx": ("S", 513, 1, 2000, 0, True),
    "W_L_512": ("L", 512, 20, 13000, 0, False), "W_L_513": ("L", 513, 20, 13000, 0, False),
    "W_B_512": ("B", 512, 1, 65600, 60, False), "W_B_513": ("B", 513, 1, 65600, 60, False),
}


def w_cells(later, n_vox, n_total, front_blocks):
    """The W sequence.  Voxel V_j: a one-point first run, another voxel's point, then exactly `later` more points of V_j: runs of 1
    and 2, then 64 + 63 from a chunk boundary on, then groups of 64 separated by one foreign point, so that each group starts one
    lane later than the one before and is cut by the chunk boundary into (63, 1), (62, 2), ...  Foreign points are each a voxel of
    their own.  Returns (cells (n, 3), the V cells)."""
    seq, filler = [], [0]
    V = [np.array([j - 10, 0, 6], np.int64) for j in range(n_vox)]

    def put_v(j, cnt):
        seq.extend([V[j]] * cnt)

    def put_f(cnt=1):
        for _ in range(cnt):
            seq.append(lattice(np.array([filler[0]]), (64, 64, 1), (-32, -32, -6))[0]); filler[0] += 1

    seq.extend(list(blocks(front_blocks, (16, 16, 1), (-8, -8, 12))))
    for j in range(n_vox):
        put_v(j, 1); put_f()                               # the first run, then "some other voxel's point"
        put_v(j, 1); put_f(); put_v(j, 2); put_f()
        put_f((-len(seq)) % 64)
        put_v(j, 64); put_v(j, 63); put_f()
        rem = later - (1 + 2 + 64 + 63)
        while rem > 0:
            g = min(64, rem)
            put_v(j, g); put_f(); rem -= g
    tail = n_total - len(seq)
    assert tail >= 0
    seq.extend(list(sweep(tail, 8, (64, 64, 4), (-32, -32, 20))))
    return np.array(seq, np.int64), np.array(V)


def _w(name):
    form, later, n_vox, n_total, front, scattered = W_SPEC[name]
    rng = _rng(name.replace("_idx", ""))                   # the scattered variant is the same cloud
    cells, V = w_cells(later, n_vox, n_total, front)
    pts = points_in(rng, cells, 0.5)
    for v in V:                                            # forward f32, reversed f32 and f64 differ in every lane, for EVERY such voxel
        k = np.flatnonzero(np.all(cells == v, axis=1))
        redraw_until(rng, pts, cells, 0.5, k,
                     lambda p: order_sensitive(p, [seq_sum(p[::-1]), p.astype(np.float64).sum(axis=0).astype(np.float32)]))
    big = n_vox if later > 512 else 0
    return _single(name, pts, 0.5, _path_for_size(form), len(np.unique(cells, axis=0)),
                   dict(n=n_total, later_max=later, n_big=big, multi_overflow=0, big_overflow=0,
                        wave_walk_rounds=(big + (4 if form == "S" else 16) - 1) // (4 if form == "S" else 16)), scattered=scattered)


# ---------------------------------------------------------------------------------------------- Z: signed zeros
def _z(name):
    nz = np.float32(-0.0)
    if name == "Z_lone_negative_zero":
        cloud = np.array([[nz, nz, nz, nz]], np.float32)
        return _single(name, cloud, 0.5, S_OK, 1, dict(n=1))
    other = points_in(_rng(name), [[3, 0, 0]], 0.5)
    cloud = np.concatenate([np.array([[nz, nz, nz, 0.75]], np.float32), other, np.array([[nz, nz, nz, -0.75]], np.float32)])
    return _single(name, cloud, 0.5, S_OK, 2, dict(n=3, multi=1, runs=3))


# ---------------------------------------------------------------------------------------------- T: leaf too small
def _t(name):
    rng = _rng(name)
    _, box, size = name.split("_")
    dims = (1290, 1290, 1290) if box == "1290" else (1291, 1290, 1290)
    origin = (-645, -645, -645)                                                           # inside +-8 190 (and +-4 094)
    inner = np.stack([rng.integers(0, d, 200) for d in dims], axis=1)
    core = np.concatenate([[[0, 0, 0]], inner, [[d - 1 for d in dims]]]) + np.asarray(origin)
    n_blocks = {"S": 0, "L": 64, "B": 1024}[size]
    pad = blocks(n_blocks, (1024, 1, 1), (-512, 0, 0))                                    # inside the box
    cells = np.concatenate([pad, core])
    ok = box == "1290"
    path = [(f, fl, why) if fl != 0 else (f, 0 if ok else 1, "served" if ok else "cells") for f, fl, why in _path_for_size(size)]
    target = points_in(rng, cells, 0.25)
    pts, off = _batch([_ordinary(rng, 1500, 0.25), target, _ordinary(rng, 900, 0.25)])
    return Case(name, pts, off, 0.25, 1, "OK" if ok else "CAPACITY", path, len(np.unique(cells, axis=0)) if ok else None,
                dict(cells=dims[0] * dims[1] * dims[2], coord_abs_max=645.0))


# ---------------------------------------------------------------------------------------------- X: coordinates no int holds
X_SPEC = {"X_pos_1e9": (0, 6.0e8), "X_neg_1e9": (1, -6.0e8), "X_pos_2p31": (2, 1.0e10), "X_neg_2p31": (0, -1.0e10)}   # axis, metres at leaf 0.5


def _x(name):
    rng = _rng(name)
    ax, metres = X_SPEC[name]
    target = points_in(rng, sweep(3000, 4, (20, 20, 20), (-10, -10, -10)), 0.5)
    target[1500, ax] = np.float32(metres)
    pts, off = _batch([_ordinary(rng, 1500, 0.5), target, _ordinary(rng, 900, 0.5)])
    path = [("S", 4, "coordinates"), ("B", 4, "coordinates"), ("G", 1, "coordinates")]
    return Case(name, pts, off, 0.5, 1, "CAPACITY", path, None, dict(coord_abs_max=float(np.float32(np.float32(abs(metres)) * np.float32(2.0)))))


# ---------------------------------------------------------------------------------------------- Q: the device-wide form's key
Q_SPEC = {"Q_64_key_bits": (65536, False), "Q_65_key_bits": (65537, False), "Q_65_key_bits_revisit": (65537, True)}   # clouds, revisit cloud
Q_TWO_POINT_CLOUD = 30000
Q_REVISIT_CLOUD = 50000
Q_REVISIT_LENS = (24, 16, 24)                              # the revisited voxel's three runs; one foreign point after the first and the second
Q_REVISIT_RUNS = (tuple(range(0, 24)), tuple(range(25, 41)), tuple(range(42, 66)))     # its points within the cloud, run by run


def q_revisit_cloud(rng, leaf):
    """66 points: a voxel visited three times (24, 16 and 24 points) with another voxel's point between the visits, drawn so
    that its sum in arrival order differs in all four lanes from its sum in each of the five other orders of its runs.  The
    keys-only sort keeps a voxel's runs in arrival order by the run number in the key; the (key, value) sort only by being stable."""
    A, F1, F2 = [2, -3, 1], [5, 5, 5], [-4, 0, 2]
    a, b, c = Q_REVISIT_LENS
    cells = np.array([A] * a + [F1] + [A] * b + [F2] + [A] * c, np.int64)
    pts = points_in(rng, cells, leaf)
    k = np.concatenate(Q_REVISIT_RUNS)
    runs = [np.arange(0, a), np.arange(a, a + b), np.arange(a + b, a + b + c)]
    others = [np.concatenate([runs[i] for i in o]) for o in itertools.permutations(range(3)) if o != (0, 1, 2)]
    redraw_until(rng, pts, cells, leaf, k, lambda p: order_sensitive(p, [seq_sum(p[o]) for o in others]))
    return pts


def _q(name):
    rng = _rng(name)
    B, revisit = Q_SPEC[name]
    clouds = [c[None] for c in points_in(rng, lattice(rng.integers(0, 8000, B), (20, 20, 20), (-10, -10, -10)), 0.5)]
    clouds[Q_TWO_POINT_CLOUD] = points_in(rng, [[-550, -550, -550], [549, 549, 549]], 0.5)     # an 1100^3 box: 1.331e9 cells, 31 bits
    if revisit:
        clouds[Q_REVISIT_CLOUD] = q_revisit_cloud(rng, 0.5)
    pts, off = _batch(clouds)
    bits = 31 + 17 + (16 if B == 65536 else 17)
    return Case(name, pts, off, 0.5, Q_TWO_POINT_CLOUD, "OK", S_OK, 2,
                dict(cell_bits=31, rid_bits=17, cloud_bits=bits - 48, key_bits=bits, pairs_sort=bits > 64))


# ---------------------------------------------------------------------------------------------- the table
_FAMILIES = {"P": lambda name: _p(name, int(name.split("_")[1])), "R": _r, "C": _c, "K": _k, "M": _m, "W": _w, "Z": _z, "T": _t, "X": _x, "Q": _q}

NAMES = (["P_%d" % n for n in P_COUNTS]
         + ["R_S_2048", "R_S_2049", "R_L_12288", "R_L_12289", "R_B_65536", "R_G_65537"]
         + ["C_%s_%s_%s_%d" % (f, a, s, m) for f, mags in (("L", (8190, 8191)), ("B", (4094, 4095))) for a in "xyz" for s in ("pos", "neg") for m in mags]
         + ["K_%s_%s" % (box, size) for box in K_BOXES for size in "SLB"]
         + ["M_S_960", "M_S_961", "M_L_3840", "M_L_3841", "M_B_3841"]
         + list(W_SPEC)
         + ["Z_lone_negative_zero", "Z_two_runs_cancel"]
         + ["T_1290_S", "T_1291_S", "T_1291_L", "T_1291_B"]
         + list(X_SPEC)
         + list(Q_SPEC))

SINGLE = [n for n in NAMES if n[0] in "PRCKMWZ"]          # one cloud, delivered: also through msfl_voxel_downsample
REFUSED = [n for n in NAMES if n[0] in "TX" and n != "T_1290_S"]


@functools.lru_cache(maxsize=6)
def case(name):
    return _FAMILIES[name[0]](name)
