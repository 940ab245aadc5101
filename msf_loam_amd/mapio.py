"""A map store on disk: one .npz holding what msfl_grid_dump_cells and msfl_grid_dump deliver, which is what
msfl_grid_load_cells takes back bit for bit.  numpy only; nothing here touches the GPU until save_grid / load_grid are
handed a capi.Grid.

The file is checked by the rules msfl_grid_load_cells applies before it stages anything, so a file the device call
would refuse is refused when it is read (MapFileError), not after a session has been built around it."""
import numpy as np

FORMAT = 1
LIM = 8192          # +-8192 cells per axis (msfl_c_api.h)
BITS = 14


class MapFileError(ValueError):
    pass


def cell_keys(cells):
    """(n, 4) {ix, iy, iz, count} -> the store's 42-bit keys: ascending in (iz, iy, ix)."""
    c = np.asarray(cells, np.int64).reshape(-1, 4)
    return ((c[:, 2] + LIM) << (2 * BITS)) | ((c[:, 1] + LIM) << BITS) | (c[:, 0] + LIM)


def validate(cells, points):
    """The argument rules of msfl_grid_load_cells, plus what its device path refuses a whole load for (a point that is not finite).
    Returns (cells int32 (n, 4), points float32 (m, 4)); raises MapFileError naming the rule."""
    cells, points = np.asarray(cells), np.asarray(points)
    if cells.ndim != 2 or cells.shape[1] != 4 or not np.issubdtype(cells.dtype, np.integer):
        raise MapFileError("cells: an (n, 4) integer array {ix, iy, iz, count} is needed, got %s %s" % (cells.dtype, cells.shape))
    if points.ndim != 2 or points.shape[1] != 4 or points.dtype != np.float32:
        raise MapFileError("points: an (m, 4) float32 array is needed, got %s %s" % (points.dtype, points.shape))
    cells = cells.astype(np.int64)
    if (cells[:, 3] <= 0).any():
        raise MapFileError("a listed cell with a count <= 0")
    if (cells[:, :3] < -LIM).any() or (cells[:, :3] >= LIM).any():
        raise MapFileError("a cell index outside [-8192, 8191]")
    if (np.diff(cell_keys(cells)) <= 0).any():
        raise MapFileError("cells not strictly ascending in (iz, iy, ix)")
    if int(cells[:, 3].sum()) != len(points):
        raise MapFileError("the counts sum to %d, the file holds %d points" % (int(cells[:, 3].sum()), len(points)))
    if not np.isfinite(points[:, :3]).all():
        raise MapFileError("a point is not finite")
    return np.ascontiguousarray(cells.astype(np.int32)), np.ascontiguousarray(points)


def write_map(path, resolution, leaf, cells, points):
    """One store as `path` (.npz): resolution and leaf of the store, its cell list and its points."""
    cells, points = validate(cells, points)
    if not (resolution > 0 and leaf > 0):
        raise MapFileError("resolution and leaf must be positive")
    with open(path, "wb") as f:
        np.savez(f, format=np.int32(FORMAT), resolution=np.float32(resolution), leaf=np.float32(leaf), cells=cells, points=points)


def read_map(path):
    """-> (resolution, leaf, cells, points), validated."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("format", "resolution", "leaf", "cells", "points") if k not in z.files]
        if missing:
            raise MapFileError("not a map file: no %s" % ", ".join(missing))
        if int(z["format"]) != FORMAT:
            raise MapFileError("map file format %d, this reader knows %d" % (int(z["format"]), FORMAT))
        resolution, leaf, cells, points = float(z["resolution"]), float(z["leaf"]), z["cells"], z["points"]
    if not (resolution > 0 and leaf > 0):
        raise MapFileError("resolution and leaf must be positive")
    cells, points = validate(cells, points)
    return resolution, leaf, cells, points


def save_grid(path, grid):
    """The whole of a capi.Grid (dump_cells + dump, with the resolution and leaf it was created with) as a map file.  Returns
    (n_cells, n_points)."""
    cells, points = grid.dump_cells(), grid.dump()
    write_map(path, grid.resolution, grid.leaf, cells, points)
    return len(cells), len(points)


def load_grid(path, grid):
    """A map file into a capi.Grid through msfl_grid_load_cells.  The cells of the file must not be live in the store, and the
    store must have the file's resolution and leaf: a slab is only a cell of a store with the same cells and the same voxels.
    Returns the GridLoadInfo."""
    r, l, cells, points = read_map(path)
    if np.float32(grid.resolution) != np.float32(r):
        raise MapFileError("the file's resolution is %g, the store's %g" % (r, grid.resolution))
    if np.float32(grid.leaf) != np.float32(l):
        raise MapFileError("the file's leaf is %g, the store's %g" % (l, grid.leaf))
    return grid.load_cells(cells, points)


# ---- place database (capi.Places) ----

PLACES_FORMAT = 1
PLACE_CONFIG_FIELDS = ("n_ring", "n_sector", "min_range", "max_range", "height_offset", "capacity")


def save_places(path, places):
    """The config and every descriptor of a capi.Places as one .npz.  Returns the number of entries."""
    desc = places.get(0, places.size())
    cfg = {k: getattr(places.config, k) for k in PLACE_CONFIG_FIELDS}
    with open(path, "wb") as f:
        np.savez(f, places_format=np.int32(PLACES_FORMAT), descriptors=desc,
                 **{k: (np.int32(v) if isinstance(v, int) else np.float64(v)) for k, v in cfg.items()})
    return len(desc)


def read_places(path):
    """-> (config dict, descriptors (n, n_ring, n_sector) float32), checked by the rules msfl_places_add_descriptors applies."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("places_format", "descriptors") + PLACE_CONFIG_FIELDS if k not in z.files]
        if missing:
            raise MapFileError("not a place file: no %s" % ", ".join(missing))
        if int(z["places_format"]) != PLACES_FORMAT:
            raise MapFileError("place file format %d, this reader knows %d" % (int(z["places_format"]), PLACES_FORMAT))
        cfg = {k: (int(z[k]) if k in ("n_ring", "n_sector", "capacity") else float(z[k])) for k in PLACE_CONFIG_FIELDS}
        desc = z["descriptors"]
    if desc.dtype != np.float32 or desc.ndim != 3 or desc.shape[1:] != (cfg["n_ring"], cfg["n_sector"]):
        raise MapFileError("descriptors: an (n, %d, %d) float32 array is needed, got %s %s" % (cfg["n_ring"], cfg["n_sector"], desc.dtype, desc.shape))
    if not (np.isfinite(desc).all() and (desc >= 0).all()):
        raise MapFileError("a descriptor value is negative or not finite")
    return cfg, np.ascontiguousarray(desc)


def load_places(path, places=None, device=0, capacity=None):
    """A place file into a capi.Places through msfl_places_add_descriptors.  places=None creates one with the file's config
    (`capacity` overrides the file's); an existing one must have the file's bins, range gate and height offset.  Returns it."""
    from . import capi
    cfg, desc = read_places(path)
    if places is None:
        if capacity is not None:
            cfg["capacity"] = int(capacity)
        places = capi.Places(device, **cfg)
    else:
        for k in PLACE_CONFIG_FIELDS[:-1]:
            if getattr(places.config, k) != cfg[k]:
                raise MapFileError("the file's %s is %r, the database's %r" % (k, cfg[k], getattr(places.config, k)))
    if len(desc):
        places.add_descriptors(desc)
    return places


# ---- keyframe store (capi.Keyframes) ----

KEYFRAMES_FORMAT = 1
KEYFRAMES_CONFIG_FIELDS = ("max_keyframes", "max_corner_points", "max_surf_points", "leaf_corner", "leaf_surf")


def _keyframes_validate(cfg, n_corner, n_surf, corner, surf):
    """The rules msfl_keyframes_create and msfl_keyframes_add apply, so that a file they would refuse is refused when it is read."""
    for name, a in (("n_corner", n_corner), ("n_surf", n_surf)):
        if a.ndim != 1 or a.dtype != np.int32:
            raise MapFileError("%s: a 1-D int32 array is needed, got %s %s" % (name, a.dtype, a.shape))
        if (a < 0).any():
            raise MapFileError("%s: a negative count" % name)
    if len(n_corner) != len(n_surf):
        raise MapFileError("n_corner lists %d keyframes, n_surf %d" % (len(n_corner), len(n_surf)))
    for name, pts, cnt in (("corner", corner, n_corner), ("surf", surf, n_surf)):
        if pts.ndim != 2 or pts.shape[1] != 4 or pts.dtype != np.float32:
            raise MapFileError("%s: an (m, 4) float32 array is needed, got %s %s" % (name, pts.dtype, pts.shape))
        if int(cnt.astype(np.int64).sum()) != len(pts):
            raise MapFileError("the %s counts sum to %d, the file holds %d points" % (name, int(cnt.astype(np.int64).sum()), len(pts)))
        if not np.isfinite(pts).all():
            raise MapFileError("a %s point is not finite" % name)
    if cfg["max_keyframes"] < 1 or cfg["max_corner_points"] < 0 or cfg["max_surf_points"] < 0:
        raise MapFileError("max_keyframes < 1 or a negative pool size")
    for k in ("leaf_corner", "leaf_surf"):
        if not (np.isfinite(cfg[k]) and cfg[k] >= 0):
            raise MapFileError("%s is negative or not finite" % k)
    if len(n_corner) > cfg["max_keyframes"] or len(corner) > cfg["max_corner_points"] or len(surf) > cfg["max_surf_points"]:
        raise MapFileError("the file holds more than its own config has room for")


def write_keyframes(path, cfg, n_corner, n_surf, corner, surf):
    """One store as `path` (.npz): its config, the counts per keyframe and the points of each kind back to back."""
    cfg = {k: (int(cfg[k]) if k.startswith("max_") else float(np.float32(cfg[k]))) for k in KEYFRAMES_CONFIG_FIELDS}
    n_corner, n_surf = np.ascontiguousarray(n_corner), np.ascontiguousarray(n_surf)
    corner, surf = np.ascontiguousarray(corner), np.ascontiguousarray(surf)
    _keyframes_validate(cfg, n_corner, n_surf, corner, surf)
    with open(path, "wb") as f:
        np.savez(f, keyframes_format=np.int32(KEYFRAMES_FORMAT), n_corner=n_corner, n_surf=n_surf, corner=corner, surf=surf,
                 **{k: (np.int32(v) if k.startswith("max_") else np.float32(v)) for k, v in cfg.items()})


def read_keyframes(path):
    """-> (config dict, n_corner, n_surf, corner, surf), validated."""
    keys = ("keyframes_format", "n_corner", "n_surf", "corner", "surf") + KEYFRAMES_CONFIG_FIELDS
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in keys if k not in z.files]
        if missing:
            raise MapFileError("not a keyframe file: no %s" % ", ".join(missing))
        if int(z["keyframes_format"]) != KEYFRAMES_FORMAT:
            raise MapFileError("keyframe file format %d, this reader knows %d" % (int(z["keyframes_format"]), KEYFRAMES_FORMAT))
        cfg = {k: (int(z[k]) if k.startswith("max_") else float(z[k])) for k in KEYFRAMES_CONFIG_FIELDS}
        n_corner, n_surf, corner, surf = z["n_corner"], z["n_surf"], z["corner"], z["surf"]
    _keyframes_validate(cfg, n_corner, n_surf, corner, surf)
    return cfg, n_corner, n_surf, np.ascontiguousarray(corner), np.ascontiguousarray(surf)


def save_keyframes(path, keyframes):
    """The config and every keyframe of a capi.Keyframes as one .npz.  Returns the number of keyframes."""
    n = keyframes.size()
    n_corner, n_surf = keyframes.sizes()
    lists = [keyframes.get(i) for i in range(n)]
    corner = np.concatenate([c for c, _ in lists]) if n else np.zeros((0, 4), np.float32)
    surf = np.concatenate([s for _, s in lists]) if n else np.zeros((0, 4), np.float32)
    write_keyframes(path, {k: getattr(keyframes.config, k) for k in KEYFRAMES_CONFIG_FIELDS}, n_corner, n_surf, corner, surf)
    return n


def load_keyframes(path, handle, keyframes=None):
    """A keyframe file into a capi.Keyframes through msfl_keyframes_add.  The file's lists are stored lists: they must not pass a
    voxel filter again, so the store they go into has both leaves 0.  keyframes=None creates one on `handle` with the file's pool
    sizes and leaves 0; an existing one must have leaves 0 itself.  Returns it; the file's config is left in `.file_config`."""
    from . import capi
    cfg, n_corner, n_surf, corner, surf = read_keyframes(path)
    if keyframes is None:
        keyframes = capi.Keyframes(handle, **dict(cfg, leaf_corner=0.0, leaf_surf=0.0))
    elif keyframes.config.leaf_corner != 0.0 or keyframes.config.leaf_surf != 0.0:
        raise MapFileError("the store filters what is added (leaves %g / %g): stored lists need leaves 0" %
                           (keyframes.config.leaf_corner, keyframes.config.leaf_surf))
    oc = np.concatenate([[0], np.cumsum(n_corner, dtype=np.int64)])
    os_ = np.concatenate([[0], np.cumsum(n_surf, dtype=np.int64)])
    for i in range(len(n_corner)):
        keyframes.add(corner[oc[i]:oc[i + 1]], surf[os_[i]:os_[i + 1]])
    keyframes.file_config = cfg
    return keyframes
