"""CPU model of msfl_search_poses (msf_loam_amd/csrc/msfl_search.cuh), restated in numpy with explicit f32 / f64 types.

TEST INFRASTRUCTURE, shared by tests/test_search_model.py (CPU) and tests/test_gpu_search.py.  Nothing here touches the GPU.

The model IS the specification (include/msfl_c_api.h, docs/kernels/search.md):
  geometry    ext = half + ceil(range / step) + dilate + 1 cells per axis, dims = 2 ext + 1, origin =
              f32((floor(t_guess / step) - ext) * step), inv = f32(1 / step); rows of ceil(dims.x / 64) + 1 words.
  voxel       floor((x - origin) * inv) per axis, both operations in f32.
  volume      one bit per voxel and kind: the finite map points inside the box; dilate = 1 adds every voxel of the box within
              Chebyshev distance 1 of a set one.
  count       yaw sample a, feature p: v = voxel(transform_point_f32(pose(a, 0), p)); p hits at (a, k) when v + k lies inside the
              box and its bit is set.  THE SHIFT IS THE DEFINITION.  Stated twice below: hits_dense looks v + k up in a dense
              boolean volume built by array slicing; hits_sparse never builds a volume: it keeps the occupied voxels as a sorted
              list of integer keys (dilation = the union of 27 shifted key lists) and asks which shifted feature keys are members.
  peaks       order (hits[0] + hits[1] descending, h ascending); h is a peak when no other hypothesis within nms_cells
              (Chebyshev on k) and nms_yaws (on a, cyclic when yaw_wraps) precedes it.  peaks_brute compares every pair;
              peaks_window is the same rule by shifted arrays, for lattices where all pairs are too many.
  candidates  the first K peaks in that order, with pose(a, k) in double.
The GPU is compared with array_equal / tobytes, no tolerance anywhere.
"""
import math
from types import SimpleNamespace

import numpy as np

from tests.score_numpy import transform_point_f32

F = np.float32
CAND_DTYPE = np.dtype([("pose", np.float64, (7,)), ("h", np.int32), ("a", np.int32), ("kx", np.int32), ("ky", np.int32),
                       ("kz", np.int32), ("hits", np.int32, (2,)), ("reserved_", np.int32)])
MAX_DIM, MAX_HYP, MAX_TABLE = 1 << 20, 1 << 24, 1 << 26
FAR = 2097152.0          # a voxel coordinate this far from the origin is never reached by a shift (and stays an exact int)


def config(**kw):
    """The defaults of msfl_search_default_config, overridden by keywords."""
    c = dict(step=0.5, half=(6, 6, 0), n_yaw=24, yaw_min=0.0, yaw_step=2.0 * 3.14159265358979323846 / 24.0, yaw_wraps=1, dilate=1,
             range=100.0, nms_cells=1, nms_yaws=1, max_volume_bytes=64 << 20)
    assert set(kw) <= set(c), kw
    c.update(kw)
    c["half"] = tuple(int(x) for x in c["half"])
    return SimpleNamespace(**c)


def geometry(guess, cfg, n_corner=0, n_surf=0):
    """msfl_search_geometry for a config it accepts."""
    guess = np.asarray(guess, np.float64)
    reach = int(math.ceil(cfg.range / cfg.step))
    ext = [cfg.half[a] + reach + cfg.dilate + 1 for a in range(3)]
    dims = [2 * e + 1 for e in ext]
    origin = np.array([F((math.floor(float(guess[a]) / cfg.step) - float(ext[a])) * cfg.step) for a in range(3)], F)
    n = [2 * cfg.half[a] + 1 for a in range(3)]
    W = (dims[0] + 63) // 64 + 1
    H = cfg.n_yaw * n[0] * n[1] * n[2]
    vol = W * dims[1] * dims[2] * 8
    nf = n_corner + n_surf
    scratch = 2 * (1 + cfg.dilate) * vol + 16 * cfg.n_yaw * nf + 16 * H + 32 * cfg.n_yaw + 56 + 88 * 1024 + 8
    return SimpleNamespace(origin=origin, inv=F(1.0 / cfg.step), dims=dims, W=W, n=n, n_yaw=cfg.n_yaw, H=H, volume_bytes=vol,
                           scratch_bytes=scratch)


def yaw_quat(guess, yaw):
    """normalised(qz(yaw) * q_guess), operation for operation what the library's host code does (libm sin / cos)."""
    hy = yaw * 0.5
    az, aw = math.sin(hy), math.cos(hy)
    bx, by, bz, bw = (float(x) for x in np.asarray(guess, np.float64)[3:])
    x, y, z, w = aw * bx - az * by, aw * by + az * bx, aw * bz + az * bw, aw * bw - az * bz
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    return np.array([x / n, y / n, z / n, w / n] if n > 0.0 else [x, y, z, w], np.float64)


def pose(guess, cfg, a, k=(0, 0, 0)):
    guess = np.asarray(guess, np.float64)
    t = [float(guess[i]) + cfg.step * float(k[i]) for i in range(3)]
    return np.concatenate([np.array(t, np.float64), yaw_quat(guess, cfg.yaw_min + float(a) * cfg.yaw_step)])


def voxel_f(p, g):
    """floor((x - origin) * inv), the two operations in f32: (n, 3) f32 in, (n, 3) f32 out (NaN / inf pass through)."""
    p = np.asarray(p, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - g.origin[None, :]).astype(F)
        return np.floor((d * g.inv).astype(F))


def map_voxels(pts, g):
    """Integer voxels (n, 3) of the finite map points inside the box."""
    f = voxel_f(np.asarray(pts, F).reshape(-1, 4)[:, :3], g)
    fin = np.isfinite(np.asarray(pts, F).reshape(-1, 4)[:, :3]).all(1)
    with np.errstate(invalid="ignore"):
        ok = fin & (f >= 0).all(1) & (f[:, 0] < g.dims[0]) & (f[:, 1] < g.dims[1]) & (f[:, 2] < g.dims[2])
    return f[ok].astype(np.int64)


def feature_voxels(guess, cfg, g, feat, a):
    """(v (n, 3) int64, valid (n,)) of one kind's features at yaw sample a."""
    feat = np.asarray(feat, F).reshape(-1, 4)[:, :3]
    fin = np.isfinite(feat).all(1)
    w = transform_point_f32(pose(guess, cfg, a), feat)
    f = voxel_f(w, g)
    with np.errstate(invalid="ignore"):
        ok = fin & (np.abs(f) < FAR).all(1)
    return np.where(ok[:, None], f, 0).astype(np.int64), ok


# ---- statement 1: a dense boolean volume, looked up at v + k ----------------------------------------------------------------------

def dense_volume(pts, g, dilate):
    vol = np.zeros((g.dims[2], g.dims[1], g.dims[0]), bool)
    v = map_voxels(pts, g)
    vol[v[:, 2], v[:, 1], v[:, 0]] = True
    if dilate:
        for axis in range(3):
            out = vol.copy()
            lo = [slice(None)] * 3; hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            out[tuple(lo)] |= vol[tuple(hi)]
            out[tuple(hi)] |= vol[tuple(lo)]
            vol = out                      # (three one-axis passes make the 3 x 3 x 3 box)
    return vol


def hits_dense(map_corner, map_surf, corner, surf, guess, cfg):
    g = geometry(guess, cfg)
    hits = np.zeros((2, g.n_yaw, g.n[2], g.n[1], g.n[0]), np.int32)
    kx = np.arange(g.n[0], dtype=np.int64) - cfg.half[0]
    for kind, (m, feat) in enumerate(((map_corner, corner), (map_surf, surf))):
        vol = dense_volume(m, g, cfg.dilate)
        for a in range(g.n_yaw):
            v, ok = feature_voxels(guess, cfg, g, feat, a)
            v = v[ok]
            for kzp in range(g.n[2]):
                z = v[:, 2] + (kzp - cfg.half[2])
                for kyp in range(g.n[1]):
                    y = v[:, 1] + (kyp - cfg.half[1])
                    row = (z >= 0) & (z < g.dims[2]) & (y >= 0) & (y < g.dims[1])
                    x = v[row, 0][:, None] + kx[None, :]
                    inside = (x >= 0) & (x < g.dims[0])
                    got = vol[z[row][:, None].repeat(g.n[0], 1)[inside], y[row][:, None].repeat(g.n[0], 1)[inside], x[inside]]
                    cnt = np.zeros(x.shape, np.int32)
                    cnt[inside] = got
                    hits[kind, a, kzp, kyp, :] = cnt.sum(0)
    return hits.reshape(2, -1)


# ---- statement 2: no volume at all, sorted integer keys of the occupied voxels ----------------------------------------------------

def _key(v, g):
    return (v[..., 2] * g.dims[1] + v[..., 1]) * g.dims[0] + v[..., 0]


def sparse_occupied(pts, g, dilate):
    v = map_voxels(pts, g)
    if dilate and len(v):
        offs = np.array([(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)], np.int64)
        v = (v[:, None, :] + offs[None, :, :]).reshape(-1, 3)
        v = v[(v >= 0).all(1) & (v[:, 0] < g.dims[0]) & (v[:, 1] < g.dims[1]) & (v[:, 2] < g.dims[2])]
    return np.unique(_key(v, g)) if len(v) else np.zeros(0, np.int64)


def hits_sparse(map_corner, map_surf, corner, surf, guess, cfg):
    g = geometry(guess, cfg)
    hits = np.zeros((2, g.H), np.int32)
    ks = np.array([(kx - cfg.half[0], ky - cfg.half[1], kz - cfg.half[2]) for kz in range(g.n[2]) for ky in range(g.n[1])
                   for kx in range(g.n[0])], np.int64)
    per_yaw = len(ks)
    dims = np.array(g.dims, np.int64)
    for kind, (m, feat) in enumerate(((map_corner, corner), (map_surf, surf))):
        occ = sparse_occupied(m, g, cfg.dilate)
        for a in range(g.n_yaw):
            v, ok = feature_voxels(guess, cfg, g, feat, a)
            v = v[ok]
            if len(v) == 0 or len(occ) == 0:
                continue
            for c0 in range(0, per_yaw, 512):                    # (chunks of shifts bound the (shift, feature) array)
                u = v[None, :, :] + ks[c0:c0 + 512, None, :]
                inside = ((u >= 0) & (u < dims)).all(-1)
                member = np.zeros(inside.shape, bool)
                member[inside] = np.isin(_key(u[inside], g), occ)
                hits[kind, a * per_yaw + c0:a * per_yaw + c0 + len(member)] = member.sum(1)
    return hits


# ---- peaks, order, candidates ------------------------------------------------------------------------------------------------------

def keys(hits):
    total = hits[0].astype(np.uint64) + hits[1].astype(np.uint64)
    return ((np.uint64(0xffffffff) - total) << np.uint64(32)) | np.arange(hits.shape[1], dtype=np.uint64)


def lattice_coords(cfg):
    n = [2 * h + 1 for h in cfg.half]
    a, kz, ky, kx = np.meshgrid(np.arange(cfg.n_yaw), np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    return a.ravel(), kx.ravel(), ky.ravel(), kz.ravel()          # primed (0-based) coordinates in hypothesis order


def peaks_brute(hits, cfg):
    """The rule, pair by pair."""
    key = keys(hits)
    a, kx, ky, kz = lattice_coords(cfg)
    out = np.zeros(len(key), bool)
    for h in range(len(key)):
        da = np.abs(a - a[h])
        if cfg.yaw_wraps:
            da = np.minimum(da, cfg.n_yaw - da)
        near = (da <= cfg.nms_yaws) & (np.abs(kx - kx[h]) <= cfg.nms_cells) & (np.abs(ky - ky[h]) <= cfg.nms_cells) & \
               (np.abs(kz - kz[h]) <= cfg.nms_cells)
        near[h] = False
        out[h] = not (key[near] < key[h]).any()
    return out


def peaks_window(hits, cfg):
    """The same rule by shifted arrays."""
    n = [2 * h + 1 for h in cfg.half]
    key = keys(hits).reshape(cfg.n_yaw, n[2], n[1], n[0])
    out = np.ones(key.shape, bool)
    if cfg.yaw_wraps:
        yaw_shifts = sorted({d % cfg.n_yaw for d in range(-cfg.nms_yaws, cfg.nms_yaws + 1)})
    else:
        yaw_shifts = [d for d in range(-cfg.nms_yaws, cfg.nms_yaws + 1) if abs(d) < cfg.n_yaw]
    c = cfg.nms_cells
    big = np.uint64(0xffffffffffffffff)
    for da in yaw_shifts:
        for dz in range(-min(c, n[2] - 1), min(c, n[2] - 1) + 1):
            for dy in range(-min(c, n[1] - 1), min(c, n[1] - 1) + 1):
                for dx in range(-min(c, n[0] - 1), min(c, n[0] - 1) + 1):
                    if dz == 0 and dy == 0 and dx == 0 and da == 0:
                        continue
                    nb = np.full(key.shape, big, np.uint64)          # nb[a, z, y, x] = key[a + da, z + dz, y + dy, x + dx], or none
                    src = np.roll(key, -da, 0) if cfg.yaw_wraps else key
                    sl_d, sl_s = [slice(None)] * 4, [slice(None)] * 4
                    for ax, d in ((1, dz), (2, dy), (3, dx)) + (() if cfg.yaw_wraps else ((0, da),)):
                        if d > 0:
                            sl_d[ax], sl_s[ax] = slice(0, -d), slice(d, None)
                        elif d < 0:
                            sl_d[ax], sl_s[ax] = slice(-d, None), slice(0, d)
                    nb[tuple(sl_d)] = src[tuple(sl_s)]
                    out &= ~(nb < key)
    return out.ravel()


def candidates(hits, guess, cfg, K, peaks=None):
    """The first K peaks in the order, as CAND_DTYPE records."""
    pk = peaks_window(hits, cfg) if peaks is None else peaks
    key = keys(hits)
    order = np.flatnonzero(pk)
    order = order[np.argsort(key[order], kind="stable")][:K]
    a, kx, ky, kz = lattice_coords(cfg)
    rec = np.zeros(len(order), CAND_DTYPE)
    for i, h in enumerate(order):
        k = (int(kx[h]) - cfg.half[0], int(ky[h]) - cfg.half[1], int(kz[h]) - cfg.half[2])
        rec[i]["pose"] = pose(guess, cfg, int(a[h]), k)
        rec[i]["h"], rec[i]["a"] = h, a[h]
        rec[i]["kx"], rec[i]["ky"], rec[i]["kz"] = k
        rec[i]["hits"] = hits[:, h]
    return rec


def search(map_corner, map_surf, corner, surf, guess, cfg, K, sparse=True):
    """Handle.search_poses(..., want_hits=True): (candidates, hits (2, H))."""
    hits = (hits_sparse if sparse else hits_dense)(map_corner, map_surf, corner, surf, guess, cfg)
    return candidates(hits, guess, cfg, K), hits
