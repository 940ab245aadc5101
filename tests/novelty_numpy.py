"""CPU model of msfl_grid_render and msfl_scan_novelty (docs/kernels/novelty.md), built from the carve's model (tests/carve_numpy.py):
the same pixels, the same inverse pose, the same range image.  `cfg` is a capi.NoveltyConfig (render also takes its `image`, a
capi.CarveConfig, alone); `tables` come from capi.carve_tables(cfg.image).  Images are (n_row, n_col) f32 and are compared and
minimised by bit pattern, as the kernels do it."""
import numpy as np

from tests import carve_numpy as cn

F = np.float32
NONE, UNSEEN, COVERED, IN_FRONT = range(4)
EMPTY = np.uint32(0x7F800000)


def _image_cfg(cfg):
    return getattr(cfg, "image", cfg)


def render(grid_model, pose, cfg, tables, image=None):
    """(image, n_tested) of a cn.CarveGrid for a sensor at `pose`: the one line of the definition, the minimum taken into `image`
    (unsigned, on the bit patterns) when one is given."""
    cfg = _image_cfg(cfg)
    dump = grid_model.dump()
    local = grid_model.o.transform_cloud(dump, cn.inverse_pose(grid_model.o, pose)) if len(dump) else dump
    img = cn.range_image(local, cfg, tables)
    n_tested = int(cn.pixels(local[:, :3], cfg, tables)[0].sum()) if len(dump) else 0
    if image is not None:
        old = np.ascontiguousarray(image, F).reshape(img.shape)
        img = np.minimum(img.view(np.uint32), old.view(np.uint32)).view(F)
    return img, n_tested


def window(img, cfg):
    """(mlim, support) per pixel: rows +-window_row clamped (a repeated edge row is counted again), columns +-window_col wrapping.
    mlim is f32 (the unsigned minimum of the bit patterns), support an int array."""
    cfg = _image_cfg(cfg)
    bits = np.ascontiguousarray(img, F).view(np.uint32)
    n_row = bits.shape[0]
    m = np.full(bits.shape, EMPTY, np.uint32)
    support = np.zeros(bits.shape, np.int64)
    for dr in range(-int(cfg.window_row), int(cfg.window_row) + 1):
        rows = np.clip(np.arange(n_row) + dr, 0, n_row - 1)
        for dc in range(-int(cfg.window_col), int(cfg.window_col) + 1):
            v = np.roll(bits[rows], -dc, axis=1)
            m = np.minimum(m, v)
            support += v != EMPTY
    return m.view(F), support


def classify(scan, img, cfg, tables):
    """uint8 class per scan point (sensor frame) against the map image."""
    scan = np.asarray(scan, F).reshape(-1, 4)
    if len(scan) == 0:
        return np.zeros(0, np.uint8)
    mlim, support = window(img, cfg)
    has, r, row, col = cn.pixels(scan[:, :3], cfg.image, tables)
    row, col = np.where(has, row, 0), np.where(has, col, 0)
    with np.errstate(all="ignore"):
        reach = (r * (F(1) + F(cfg.image.margin_rel))) + F(cfg.image.margin_abs)
        assert reach.dtype == F
        front = reach < mlim[row, col]
    cls = np.where(support[row, col] < int(cfg.min_support), UNSEEN, np.where(front, IN_FRONT, COVERED))
    return np.where(has, cls, NONE).astype(np.uint8)


def mask(scan, cls, keep_classes):
    """masked_out: the points of a dropped class get x = y = z = NaN (bits 0x7fc00000), the fourth field stays."""
    out = np.array(np.asarray(scan, F).reshape(-1, 4), copy=True)
    drop = ((int(keep_classes) >> cls.astype(np.int64)) & 1) == 0
    out.view(np.uint32)[drop, :3] = 0x7FC00000
    return out


def info(cls, img, keep_classes):
    """(n_class x 4, n_map_pixels, n_kept, applied) as NoveltyInfo.as_tuple() gives it."""
    n_class = tuple(int((cls == k).sum()) for k in range(4))
    kept = int((((int(keep_classes) >> cls.astype(np.int64)) & 1) == 1).sum())
    return (n_class, int((np.ascontiguousarray(img, F).view(np.uint32) != EMPTY).sum()), kept, 1)
