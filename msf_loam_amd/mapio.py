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
