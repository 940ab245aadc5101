"""The dense-wall scene of the novelty tests (tests/test_novelty_model.py checks its preconditions on the CPU,
tests/test_gpu_novelty.py runs it on the device, tests/cpp/novelty_check.cpp builds the same scene at the identity pose).

A coarse image of 36 x 4 pixels over -16 .. +16 degrees (columns of 10 degrees, rows of 8).  The map holds one point at the centre
direction of every pixel, 10 m from the sensor, except in a block of 7 adjacent columns (14 .. 20, across the half-turn seam at
column 18) that is left empty: with window_col = 2 the three columns in its middle see an empty window, with window_col = 0 all
seven do.  Neighbouring map points lie 1.4 m or more apart, so a 0.2 m leaf merges none of them.  The scan, in three parts:
  covered   the map's own directions at 10 m
  in front  a patch of them (columns 2 .. 5, rows 1 .. 2) at 4 m
  unseen    the directions of the block's three middle columns at 6 m"""
import numpy as np

F = np.float32
N_COL, N_ROW = 36, 4
BLOCK = range(14, 21)
MIDDLE = range(16, 19)
PATCH_COLS, PATCH_ROWS = range(2, 6), range(1, 3)
LEAF = 0.2

POSE = np.array([4.0, -7.5, 1.25, 0.02, -0.03, 0.25, 0.0])
POSE[6] = np.sqrt(1.0 - (POSE[3:6] ** 2).sum())


def config(capi, window_col=2, **kw):
    return capi.novelty_config(n_col=N_COL, n_row=N_ROW, window_col=window_col, window_row=1, **kw)


def _rays(cols, rows, r):
    pts = []
    for row in rows:
        for col in cols:
            az, el = np.deg2rad((col + 0.5) * 360.0 / N_COL), np.deg2rad(-16.0 + (row + 0.5) * 32.0 / N_ROW)
            pts.append([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)])
    out = np.zeros((len(pts), 4), F)
    out[:, :3] = np.array(pts)
    out[:, 3] = np.arange(len(pts)) / 1000.0
    return out


def wall_cols():
    return [c for c in range(N_COL) if c not in BLOCK]


def map_points_sensor():
    """The wall in the sensor frame, (116, 4) f32."""
    return _rays(wall_cols(), range(N_ROW), 10.0)


def scan_parts():
    """(covered, in front, unseen): the three parts of the scan, sensor frame."""
    return _rays(wall_cols(), range(N_ROW), 10.0), _rays(PATCH_COLS, PATCH_ROWS, 4.0), _rays(MIDDLE, range(N_ROW), 6.0)


def scan():
    return np.concatenate(scan_parts())


def expected():
    """The class of every point of scan()."""
    a, b, c = scan_parts()
    return np.concatenate([np.full(len(a), 2), np.full(len(b), 3), np.full(len(c), 1)]).astype(np.uint8)
