"""The shapes the pose search is held to, shared by tests/test_search_model.py (the two model statements against each other, CPU)
and tests/test_gpu_search.py (the kernels against the model).  TEST INFRASTRUCTURE; nothing here touches the GPU.

Every case is (map_corner, map_surf, corner, surf, guess, cfg, K).  The shapes are the smallest at which a mechanism can break:
range 3 m at pitch 0.5 m gives a box of some twenty voxels a side, so a row is one data word (or three with half[0] = 64) and a
feature beyond `range` has a window hanging over the row's end or a y / z shift that leaves the box."""
import numpy as np

from msf_loam_amd import synth
from tests import search_numpy as sn

F = np.float32
GUESS = np.array([3.3, -7.2, 1.1, 0.05, -0.03, 0.3, 0.95])
GUESS[3:] /= np.linalg.norm(GUESS[3:])


def _pts(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.zeros((len(xyz), 1), F)], 1)


def _cloud(rng, n, centre, half):
    return _pts(np.asarray(centre, np.float64)[None, :] + rng.uniform(-half, half, (n, 3)))


def random_case(seed, n_map=(150, 400), n_feat=(40, 70), guess=GUESS, K=16, **cfg_kw):
    """Map points in a cube a little larger than the box; features in the sensor frame out to 1.6 x range."""
    cfg_kw.setdefault("range", 3.0)
    cfg_kw.setdefault("half", (2, 2, 0))
    cfg_kw.setdefault("n_yaw", 3)
    cfg_kw.setdefault("yaw_step", 0.4)
    cfg_kw.setdefault("yaw_wraps", 0)
    cfg = sn.config(**cfg_kw)
    rng = np.random.default_rng(seed)
    reach = cfg.range + cfg.step * (max(cfg.half) + 4)
    return (_cloud(rng, n_map[0], guess[:3], reach), _cloud(rng, n_map[1], guess[:3], reach),
            _cloud(rng, n_feat[0], (0, 0, 0), 1.6 * cfg.range), _cloud(rng, n_feat[1], (0, 0, 0), 1.6 * cfg.range), np.array(guess), cfg, K)


def _with(case, **kw):
    mc, ms, c, s, guess, cfg, K = case
    return (kw.get("mc", mc), kw.get("ms", ms), kw.get("c", c), kw.get("s", s), kw.get("guess", guess), kw.get("cfg", cfg), kw.get("K", K))


def _handmade(dilate):
    """Five points per kind: duplicates in one voxel, a point exactly on a voxel face, negative coordinates (floor, not truncation),
    and one in each outermost voxel of the box; two features in one voxel; the guess at the origin with the identity rotation."""
    guess = np.array([0.2, -0.2, 0.1, 0, 0, 0, 1.0])
    cfg = sn.config(range=3.0, half=(2, 1, 1), n_yaw=2, yaw_step=np.pi / 2, yaw_wraps=0, dilate=dilate, nms_cells=1, nms_yaws=0)
    g = sn.geometry(guess, cfg)
    lo = g.origin.astype(np.float64)
    hi = lo + cfg.step * (np.array(g.dims) - 1)
    m = _pts([[0.26, 0.26, 0.26], [0.27, 0.3, 0.49], [-0.5, -1.0, 0.0], lo + 0.01, hi + 0.25])
    m2 = _pts([[-0.01, -0.01, -0.01], [-0.49, -0.3, -0.2], [1.0, 1.5, -1.5], lo, hi + 0.49])
    c = _pts([[0.1, 0.5, 0.2], [0.12, 0.52, 0.22], [-0.7, -0.8, 0.1], hi - guess[:3], lo - guess[:3]])
    s = _pts([[-0.21, 0.19, -0.11], [-0.22, 0.18, -0.12], [0.8, 1.7, -1.6], [2.9, 2.9, -2.9], [-4.6, 0.0, 0.0]])
    return m, m2, c, s, guess, cfg, 16


def _nonfinite():
    case = random_case(7, n_map=(60, 80), n_feat=(20, 30))
    mc, ms, c, s = (x.copy() for x in case[:4])
    mc[3, 0] = np.nan; mc[10, 2] = np.inf; ms[0, 1] = -np.inf; ms[79, :3] = np.nan
    c[0, 0] = np.nan; c[19, 1] = np.inf; s[5, 2] = -np.inf; s[6, :3] = np.nan
    c[7, :3] = 3e38; s[8, :3] = -3e38                   # finite, but the transform or the voxel is not
    return _with(case, mc=mc, ms=ms, c=c, s=s)


def _empty_map(n_c, n_s):
    case = random_case(11, n_map=(0, 0))
    return _with(case, mc=case[0][:n_c], ms=case[1][:n_s])


def _counts(n_map):
    case = random_case(12, n_map=(5, 5), n_feat=(6, 9))
    return _with(case, mc=case[0][:n_map], ms=case[1][:n_map])


CASES = {
    "random": lambda: random_case(1),
    "random_no_dilate": lambda: random_case(2, dilate=0),
    "map_0": lambda: _counts(0),
    "map_1": lambda: _counts(1),
    "map_5": lambda: _counts(5),
    "map_corner_only": lambda: _with(random_case(13), ms=random_case(13)[1][:0]),
    "handmade_dilate0": lambda: _handmade(0),
    "handmade_dilate1": lambda: _handmade(1),
    "nonfinite": _nonfinite,
    "far_guess": lambda: random_case(3, guess=np.concatenate([[5000.0, -3000.0, 20.0], GUESS[3:]])),
    "negative_box": lambda: random_case(4, guess=np.concatenate([[-12.3, -0.2, -5.1], GUESS[3:]])),
    "yaw_1": lambda: random_case(5, n_yaw=1),
    "yaw_2_z_2": lambda: random_case(6, n_yaw=2, half=(1, 2, 2)),
    "lattice_67240": lambda: random_case(8, n_feat=(1, 2), half=(20, 20, 0), n_yaw=40, yaw_step=2 * np.pi / 40, yaw_wraps=1, K=1024),
}
for _n in (0, 1, 63, 64, 65, 255, 256, 257):
    CASES["features_%d" % _n] = (lambda n: lambda: random_case(20 + n, n_feat=(n, n), half=(3, 1, 0), n_yaw=2))(_n)
# the correlate kernel's carry-save counters hold 255 masks a lane and a lane adds one mask per 64 features of a kind: the flush
# inside the feature loop first runs at 255 x 64 = 16 320 features of one kind (exactly at the loop's end there, mid-loop at
# 16 321), twice at 32 641; the map is dense, so most counts are far above 255
for _n in (16320, 16321, 32641):
    CASES["flush_%d" % _n] = (lambda n: lambda: random_case(90 + n % 7, n_map=(3000, 3000), n_feat=(n, 5) if n % 2 else (5, n), half=(3, 1, 0),
                                                            n_yaw=2))(_n)
for _hx in (0, 31, 32, 63, 64):
    CASES["half_x_%d" % _hx] = (lambda hx: lambda: random_case(40 + hx, n_feat=(30, 50), half=(hx, 1, 0), n_yaw=2, K=64))(_hx)

# peaks and top-K: (windows, wrap, K) over one lattice with many equal totals (few map points, dilated: totals of 0, 1, 2)
PEAK_CASES = {}
for _cells, _yaws, _wraps, _K in ((0, 0, 0, 16), (0, 0, 1, 1024), (1, 1, 0, 16), (1, 1, 1, 16), (2, 2, 1, 1), (2, 1, 0, 1024), (1, 2, 1, 7),
                                  (0, 2, 1, 16), (2, 0, 0, 16), (1, 5, 1, 16)):
    PEAK_CASES["cells%d_yaws%d_wrap%d_K%d" % (_cells, _yaws, _wraps, _K)] = (
        lambda c, y, w, K: lambda: random_case(60, n_map=(3, 4), n_feat=(9, 12), half=(3, 2, 1), n_yaw=6, yaw_step=2 * np.pi / 6, yaw_wraps=w,
                                               nms_cells=c, nms_yaws=y, K=K))(_cells, _yaws, _wraps, _K)
PEAK_CASES["all_zero"] = lambda: _with(random_case(61, n_map=(0, 0), half=(3, 2, 1), n_yaw=6, yaw_wraps=1, K=1024))
PEAK_CASES["all_zero_no_window"] = lambda: _with(random_case(61, n_map=(0, 0), half=(3, 2, 1), n_yaw=6, nms_cells=0, nms_yaws=0, K=1024))
PEAK_CASES["busy_K1"] = lambda: random_case(62, K=1)
PEAK_CASES["busy_K1024"] = lambda: random_case(62, nms_cells=0, nms_yaws=0, K=1024)


def yawed(pose, yaw, dx, dy):
    """examples/score_lattice.py: `pose` moved by (dx, dy) and turned by yaw about the world's z axis."""
    out = np.array(pose, np.float64)
    out[0] += dx; out[1] += dy
    q = synth.quat_mul(np.array([0.0, 0.0, np.sin(yaw / 2.0), np.cos(yaw / 2.0)]), out[3:])
    out[3:] = q / np.linalg.norm(q)
    return out


FIXTURE_RANGE = {"room": 40.0, "outdoor": 75.0}      # the scans' 99th-percentile feature range is 38.8 m / 72.5 m

_fixtures = {}


def fixture(kind):
    """The fixture of examples/score_lattice.py: the world's map, the scan of seeds SEED + 5 / + 6 at the true pose, and a guess
    (1.2, -0.9) m and 34 degrees off; pitch 0.5, 24 yaws, half {4, 4, 0}, dilate 1.  -> dict, computed once per process."""
    if kind not in _fixtures:
        world = synth.World(ground_half=synth.ground_half_for_target(50000)) if kind == "room" else synth.World(kind=kind)
        mc, ms = synth.make_map(world)
        truth = (synth.random_poses(1, synth.SEED + 5) if kind == "room" else synth.world_poses(world, 1, synth.SEED + 5))[0]
        pts, _, k = synth.make_scan(world, truth, synth.SEED + 6, with_kind=True)
        corner, surf = synth.direct_features(pts, k)
        guess = yawed(truth, -np.deg2rad(34.0), 1.2, -0.9)
        cfg = sn.config(half=(4, 4, 0), range=FIXTURE_RANGE[kind])
        _fixtures[kind] = dict(mc=mc, ms=ms, corner=corner, surf=surf, truth=truth, guess=guess, cfg=cfg)
    return _fixtures[kind]
