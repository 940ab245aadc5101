"""Scenes for the carve tests (tests/test_carve_model.py on the CPU model, tests/test_gpu_grid_carve.py on the device).

hand_scene(): a scan and stored points built in the sensor frame for the default configuration (720 x 16 pixels, one beam per row),
every scan ray at the centre of its pixel:
  * a wall at x = 10 m over the azimuths +-40 deg, all 16 beams;
  * a cylinder of returns at 12 m over the azimuths -70 .. -50 deg whose column at -60 deg returns 3 m instead (a pole);
  * ground 1.5 m below the sensor over the azimuths 100 .. 140 deg, the eight beams that look down.
Every stored point carries its label in the fourth channel (class + index / 100) and lies 0.8 m or more from every other, so no
voxel of 0.2 or 0.4 m merges two of them and a stored centroid is the point itself."""
import numpy as np

F = np.float32

# label classes
BLOB, WALL, BEHIND, EMPTY_PIXEL, OUT_OF_VIEW, TOO_NEAR, NEAR_GONE, TOO_FAR, MARGIN_KEPT, MARGIN_GONE, BESIDE_POLE, FAR_GROUND, NEAR_GROUND = range(1, 14)

HAND_POSE = np.array([4.0, -7.5, 1.25, 0.02, -0.03, 0.25, 0.0])
HAND_POSE[6] = np.sqrt(1.0 - (HAND_POSE[3:6] ** 2).sum())


def _ray(az_deg, el_deg, r):
    az, el = np.deg2rad(az_deg), np.deg2rad(el_deg)
    return np.array([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)])


def hand_scan():
    """The scan, sensor frame, (n, 4) f32."""
    beams = np.arange(-15.0, 16.0, 2.0)
    pts = []
    for col in list(range(0, 80)) + list(range(640, 720)):                  # the wall at x = 10
        az = (col + 0.5) * 0.5
        for el in beams:
            pts.append(_ray(az, el, 10.0 / (np.cos(np.deg2rad(az)) * np.cos(np.deg2rad(el)))))
    for col in range(580, 620):                                              # the cylinder at 12 m, the pole at 3 m
        for el in beams:
            pts.append(_ray((col + 0.5) * 0.5, el, 3.0 if col == 600 else 12.0))
    for col in range(200, 280):                                              # the ground
        for el in beams[beams < 0]:
            pts.append(_ray((col + 0.5) * 0.5, el, 1.5 / np.sin(np.deg2rad(-el))))
    out = np.zeros((len(pts), 4), F)
    out[:, :3] = np.array(pts)
    return out


def hand_points():
    """The stored points, sensor frame, (m, 4) f32 with the label in the fourth channel."""
    rows = []

    def add(cls, pts):
        for j, p in enumerate(pts):
            rows.append([p[0], p[1], p[2], cls + j / 100.0])

    add(BLOB, [(5.0, y, z) for y in (-0.8, 0.0, 0.8) for z in (-0.75, 0.05, 0.85)])
    add(WALL, [(10.0, y, z) for y in (-3.0, -1.0, 1.0, 3.0) for z in (-1.0, 1.0)])
    add(BEHIND, [(13.0, y, 0.1) for y in (-2.0, 0.0, 2.0)])
    add(EMPTY_PIXEL, [(0.1, 5.0, 0.1), (-0.2, 6.0, 0.6)])                     # no return at azimuth 90 deg
    add(OUT_OF_VIEW, [(5.0, 0.4, 3.5), (5.0, -0.4, -3.5)])                    # elevations +-35 deg, in front of the wall
    add(TOO_NEAR, [(0.2, 0.01, 0.01)])                                       # r = 0.2 < min_range
    add(NEAR_GONE, [(1.0, 0.05, 0.03)])
    add(TOO_FAR, [(150.0, 1.0, 2.0)])                                        # r > max_range
    add(MARGIN_KEPT, [_ray(0.25, 1.0, 9.8)])                                 # 9.8 * 1.02 + 0.3 > 10.0015
    add(MARGIN_GONE, [_ray(0.25, 3.0, 9.0)])                                 # 9.0 * 1.02 + 0.3 < 10.0
    add(BESIDE_POLE, [_ray(300.75, 1.0, 6.0)])                               # column 601: 12 m behind it, the pole at 3 m one column over
    add(FAR_GROUND, [(50.0 * np.cos(np.deg2rad(120.25)), 50.0 * np.sin(np.deg2rad(120.25)), -1.5)])      # elevation -1.72 deg: the row of the -1 deg beam (85.9 m)
    add(NEAR_GROUND, [(20.0 * np.cos(np.deg2rad(120.25)), 20.0 * np.sin(np.deg2rad(120.25)), -1.5)])
    return np.array(rows, F)


def classes(pts):
    """Label class of stored points -> how many of each are present."""
    c = np.floor(np.asarray(pts)[:, 3] + 0.001).astype(int)
    return {int(k): int((c == k).sum()) for k in np.unique(c)}


def hand_expected(window_col=1, window_row=1):
    """Classes (and counts) that survive a carve of the hand scene."""
    want = {WALL: 8, BEHIND: 3, EMPTY_PIXEL: 2, OUT_OF_VIEW: 2, TOO_NEAR: 1, TOO_FAR: 1, MARGIN_KEPT: 1, NEAR_GROUND: 1}
    if window_col >= 1:
        want[BESIDE_POLE] = 1
    if window_row >= 1:
        want[FAR_GROUND] = 1
    return want
