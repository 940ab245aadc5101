"""GPU: the place database (msfl_places_*) against the numpy model of its definition (tests/place_numpy.py).

Descriptors, ring keys, indices, shifts, ring_key_d2 and n_columns are compared with array_equal; `distance` with atol = 1e-12.
That bound is derived: dot products and sums are IEEE adds and multiplies of identical operands in identical order on both
sides, so only the f64 square root and division can differ, and each of at most 120 terms in [0, 2] then moves by a few 2^-52.
Wherever an index or a shift is compared, the model's distances involved are first asserted to be bit-equal or more than 1e-9
apart.  The largest deviation seen is printed (run with -s)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import place_numpy as pn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-12
GAP = 1e-9
_worst = [0.0]


# ---- cases (built once, never modified) --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def world_scans(n=20):
    w = synth.World()
    poses = synth.random_poses(n, synth.SEED + 40)
    return tuple(synth.make_scan(w, poses[i], 100 + i)[0] for i in range(n))


@functools.lru_cache(maxsize=None)
def query_scans(n=5):
    """Revisits of the first n places: 0.5 m / 0.3 m off, yawed."""
    w = synth.World()
    poses = synth.random_poses(n, synth.SEED + 40)
    out = []
    for i in range(n):
        p = poses[i].copy()
        p[0] += 0.5
        p[1] += 0.3
        q = synth.quat_mul(p[3:], synth.quat_from_rotvec([0.0, 0.0, np.deg2rad(36.0 * (i + 1))]))
        p[3:] = q / np.linalg.norm(q)
        out.append(synth.make_scan(w, p, 900 + i)[0])
    return tuple(out)


def salted_cloud(cfg, seed=7, n=20000):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), np.float32)
    p[:, 0:2] = rng.uniform(-90, 90, (n, 2))
    p[:, 2] = rng.uniform(-3, 5, n)
    salt = []
    for c in range(3):                                     # NaN / inf in each coordinate
        for bad in (np.nan, np.inf, -np.inf):
            q = np.array([3.0, 4.0, 1.0, 0.0], np.float32)
            q[c] = bad
            salt.append(q)
    for k in range(cfg.n_ring + 1):                        # on every ring edge: x * x is compared with the f32 table entry
        x = np.float32(np.sqrt(np.float64(cfg.e2[k])))
        for xx in (x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(1e9))):
            salt.append([xx, 0.0, 1.0, 0.0])
            salt.append([0.0, -xx, 1.0, 0.0])
    for r in (0.2, 0.3, 1.0, 7.5, 33.0):                   # both axes, the diagonals, -0.0 components
        for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            salt.append([sx * r, sy * r, 0.5, 0.0])
        salt.append([r, -0.0, 0.5, 0.0])
        salt.append([-r, -0.0, 0.5, 0.0])
        salt.append([-0.0, r, 0.5, 0.0])
        salt.append([-0.0, -r, 0.5, 0.0])
    for z in (-5.0, 0.0, 3.0):                             # the origin
        salt.append([0.0, 0.0, z, 0.0])
        salt.append([-0.0, -0.0, z, 0.0])
    off = np.float32(cfg.height_offset)                    # z + offset <= 0, and just above
    for z in (-off, np.nextafter(-off, np.float32(-10)), np.nextafter(-off, np.float32(10)), np.float32(-100.0)):
        salt.append([5.0, 5.0, z, 0.0])
    salt = np.asarray(salt, np.float32)
    at = rng.choice(n, len(salt), replace=False)
    p[at] = salt
    return p


@functools.lru_cache(maxsize=None)
def describe_cases():
    base = world_scans()[0]
    assert len(base) > 8193
    clouds = [base[:n] for n in (0, 1, 255, 256, 257, 8191, 8192, 8193)] + [world_scans()[1], salted_cloud(pn.Config())]
    return tuple(clouds)


@functools.lru_cache(maxsize=None)
def big_db():
    """300 descriptors: 20 world scans, then np.roll-ed and randomly thinned copies."""
    cfg = pn.Config()
    base = [pn.describe(cfg, s) for s in world_scans()]
    rng = np.random.default_rng(11)
    out = list(base)
    while len(out) < 300:
        d = base[int(rng.integers(20))]
        if len(out) % 3 == 0:
            d = np.roll(d, int(rng.integers(1, 60)), axis=1)
        else:
            d = np.roll(d, int(rng.integers(0, 60)), axis=1) * (rng.uniform(size=d.shape) < rng.uniform(0.5, 0.95))
        out.append(np.ascontiguousarray(d, np.float32))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def query_descs():
    cfg = pn.Config()
    return np.stack([pn.describe(cfg, s) for s in query_scans()])


# ---- comparison ---------------------------------------------------------------------------------------------------------

def model_query(q, C, max_index=None, n_prefilter=0, k=1):
    """The model's answer, after asserting that its indices and shifts are decidable: distances bit-equal or > GAP apart."""
    m = pn.query(q, C, max_index, n_prefilter, k)
    assert pn.separated(m["all_distance"], GAP), "candidate distances too close for an index comparison: choose another seed"
    for i in m["index"]:
        if i >= 0:
            d, _ = pn.distances(q, np.asarray(C)[i][None])
            rest = d[0][np.isfinite(d[0]) & (d[0] != d[0].min())]          # the minimum decides the shift: bit-equal to it, or clear of it
            assert np.all(rest > d[0].min() + GAP), "shift distances too close for a shift comparison: choose another seed"
    return m


def check(rec, models):
    rec = np.asarray(rec)
    assert rec.shape == (len(models), len(models[0]["index"]))
    for row, m in zip(rec, models):
        for f in ("index", "shift", "ring_key_d2", "n_columns"):
            assert np.array_equal(row[f], m[f]), (f, row[f], m[f])
        inf = np.isinf(m["distance"])
        assert np.array_equal(np.isinf(row["distance"]), inf) and np.all(row["distance"][inf] > 0)
        if (~inf).any():
            dev = float(np.abs(row["distance"][~inf] - m["distance"][~inf]).max())
            _worst[0] = max(_worst[0], dev)
            print("place distance deviation: %.3e (largest so far %.3e)" % (dev, _worst[0]))
            assert dev <= ATOL, dev


@pytest.fixture()
def places(gpu):
    from msf_loam_amd import capi
    made = []

    def make(**cfg):
        cfg.setdefault("capacity", 512)
        p = capi.Places(0, **cfg)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


def _offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return off


# ---- describe -----------------------------------------------------------------------------------------------------------

def test_describe_batch_single_and_device_equal_the_model(places):
    import torch
    cfg = pn.Config()
    clouds = describe_cases()
    want = np.stack([pn.describe(cfg, c) for c in clouds])
    a, b, c = places(), places(), places()
    assert a.add(list(clouds)) == 0 and a.size() == len(clouds)
    for i, cl in enumerate(clouds):
        assert b.add(cl) == i
    stream = torch.cuda.Stream()
    c.set_stream(stream.cuda_stream)
    pts = torch.from_numpy(np.concatenate(clouds)).to("cuda:0")
    torch.cuda.synchronize()
    assert c.add_device(pts, _offsets(clouds)) == 0
    c.synchronize()
    for p in (a, b, c):
        d, rk = p.get(0, len(clouds), want_ring_key=True)
        assert np.array_equal(d, want)
        assert np.array_equal(rk, pn.ring_key(want))
    assert (want[0] == 0).all() and np.count_nonzero(want[1]) <= 1 and np.count_nonzero(want[-1]) > 1000
    # a window of a longer point array: offsets that do not start at 0
    d = places()
    allp, off = np.concatenate(clouds), _offsets(clouds)
    assert d.add(allp, off[5:9]) == 0
    assert np.array_equal(d.get(), want[5:8])


def test_describe_non_default_config(places):
    kw = dict(n_ring=8, n_sector=12, max_range=10.0, min_range=0.0, height_offset=1.5)
    cfg = pn.Config(**kw)
    clouds = [salted_cloud(cfg, seed=8, n=9000), world_scans()[2], world_scans()[3][:100]]
    p = places(**kw)
    p.add(clouds)
    want = np.stack([pn.describe(cfg, c) for c in clouds])
    d, rk = p.get(want_ring_key=True)
    assert np.array_equal(d, want) and np.array_equal(rk, pn.ring_key(want))
    assert np.count_nonzero(want[0]) > 50
    q = p.query(clouds[1], k=3)
    check(q, [model_query(want[1], want, k=3)])


# ---- round trip ---------------------------------------------------------------------------------------------------------

def test_round_trip_through_descriptors_and_file(places, tmp_path):
    from msf_loam_amd import mapio
    clouds = list(world_scans()[:6]) + [np.zeros((0, 4), np.float32)]
    a = places()
    a.add(clouds)
    d, rk = a.get(want_ring_key=True)
    b = places()
    assert b.add_descriptors(d) == 0
    path = str(tmp_path / "places.npz")
    assert mapio.save_places(path, a) == len(clouds)
    c = mapio.load_places(path, capacity=64)
    try:
        assert c.config.capacity == 64 and c.config.n_sector == 60
        qa = a.query(list(query_scans()[:3]), k=4)
        for other in (b, c):
            d2, rk2 = other.get(want_ring_key=True)
            assert np.array_equal(d2, d) and np.array_equal(rk2, rk)
            assert other.query(list(query_scans()[:3]), k=4).tobytes() == qa.tobytes()
    finally:
        c.close()


# ---- query --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2])
def test_query_small_databases(places, n):
    cfg = pn.Config()
    p = places()
    p.add(list(world_scans()[:n]))
    C = np.stack([pn.describe(cfg, s) for s in world_scans()[:n]])
    got = p.query(list(query_scans()), k=3)                # k beyond the candidates: -1 / +inf slots
    check(got, [model_query(q, C, k=3) for q in query_descs()])
    assert (got["index"][:, n:] == -1).all() and np.isinf(got["distance"][:, n:]).all()


def test_query_300_entries_prefilter_and_max_index(places):
    C, Q = big_db(), query_descs()
    N = len(C)
    p = places()
    assert p.add_descriptors(C) == 0 and p.size() == N
    scans = list(query_scans())
    for npre in (0, 1, 7, N, N + 5):
        check(p.query(scans, n_prefilter=npre, k=5), [model_query(q, C, n_prefilter=npre, k=5) for q in Q])
    for mi in (0, 1, N):
        check(p.query(scans, max_index=mi, k=2), [model_query(q, C, max_index=mi, k=2) for q in Q])
    mis = [0, 1, 150, 299, 300]
    check(p.query(scans, max_index=mis, n_prefilter=7, k=64), [model_query(q, C, max_index=m, n_prefilter=7, k=64) for q, m in zip(Q, mis)])
    assert p.query(scans, k=5).tobytes() == p.query(scans, max_index=N, k=5).tobytes()      # a NULL max_index: every entry
    # batch == single calls
    both = p.query(scans, n_prefilter=7, k=5)
    for i, s in enumerate(scans):
        assert p.query(s, n_prefilter=7, k=5).tobytes() == both[i:i + 1].tobytes()


def test_query_ties_rolls_and_empty_descriptors(places):
    cfg = pn.Config()
    D = pn.describe(cfg, world_scans()[4])
    other = pn.describe(cfg, world_scans()[5])
    zero = np.zeros_like(D)
    C = np.stack([other, D, zero, D, np.roll(D, 7, axis=1), np.roll(D, 53, axis=1)])
    p = places()
    p.add_descriptors(C)
    got = p.query(world_scans()[4], k=6)
    m = model_query(D, C, k=6)
    check(got, [m])
    g = got[0]
    assert g["index"].tolist()[:4] == [1, 3, 4, 5] and g["shift"].tolist()[:4] == [0, 0, 7, 53]
    assert g["distance"][0] == g["distance"][1] == g["distance"][2] == g["distance"][3]     # bit-equal: ordered by index
    assert g["index"][5] == 2 and np.isinf(g["distance"][5]) and g["n_columns"][5] == 0 and g["shift"][5] == 0
    # an all-zero query: +inf to everything, candidates in index order
    z = p.query(np.zeros((0, 4), np.float32), k=3)
    check(z, [model_query(zero, C, k=3)])
    assert z[0]["index"].tolist() == [0, 1, 2] and np.isinf(z[0]["distance"]).all() and (z[0]["n_columns"] == 0).all()


def test_query_entries_equals_query_by_points(places):
    scans = list(world_scans()[:12])
    p = places()
    p.add(scans)
    for npre in (0, 4):
        e = p.query_entries([3, 11, 0], max_index=[3, 11, 0], n_prefilter=npre, k=3)
        s = p.query([scans[3], scans[11], scans[0]], max_index=[3, 11, 0], n_prefilter=npre, k=3)
        assert e.tobytes() == s.tobytes()
    full = p.query_entries(7, k=2)
    assert full[0]["index"][0] == 7 and full[0]["shift"][0] == 0 and abs(full[0]["distance"][0]) < 1e-15


def test_query_right_after_an_asynchronous_add_sees_the_new_entries(places):
    import torch
    from msf_loam_amd import capi
    cfg = pn.Config()
    scans = list(world_scans()[:4])
    C = np.stack([pn.describe(cfg, s) for s in scans])
    p = places()
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    p.add(scans[:2])
    pts = torch.from_numpy(np.concatenate(scans[2:])).to("cuda:0")
    qpts = torch.from_numpy(np.concatenate(query_scans()[:3])).to("cuda:0")
    out = torch.zeros(3 * 4 * capi.PLACE_MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert p.add_device(pts, _offsets(scans[2:])) == 2
    p.query_device(qpts, _offsets(query_scans()[:3]), out, k=4)
    p.synchronize()
    got = out.cpu().numpy().view(capi.PLACE_MATCH_DTYPE).reshape(3, 4)
    check(got, [model_query(q, C, k=4) for q in query_descs()[:3]])
    assert p.size() == 4


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_database_unchanged(places):
    import torch
    from msf_loam_amd import capi
    scans = list(world_scans()[:3])
    p = places(capacity=4)
    p.add(scans)
    before = p.get()
    s0 = scans[0]
    bad, cap = (capi.BAD_ARG,), (capi.CAPACITY,)

    def unchanged():
        assert p.size() == 3 and np.array_equal(p.get(), before)

    for k in (0, -1, 65):
        assert p.query(s0, k=k, allow=bad) == capi.BAD_ARG
        assert p.query_entries(0, k=k, allow=bad) == capi.BAD_ARG
    assert p.query(s0, n_prefilter=-1, allow=bad) == capi.BAD_ARG
    assert p.query_entries(0, n_prefilter=-1, allow=bad) == capi.BAD_ARG
    dec = np.array([0, 100, 50], np.int32)
    assert p.add(s0, dec, allow=bad) == capi.BAD_ARG
    assert p.query(s0, dec, allow=bad) == capi.BAD_ARG
    for e in (-1, 3, 4):
        assert p.query_entries(e, allow=bad) == capi.BAD_ARG
    for mi in (-1, 4):
        assert p.query(s0, max_index=mi, allow=bad) == capi.BAD_ARG
        assert p.query_entries(0, max_index=mi, allow=bad) == capi.BAD_ARG
    unchanged()
    for v in (-1.0, np.nan, np.inf, -np.inf):
        d = before[:1].copy()
        d[0, 3, 5] = v
        assert p.add_descriptors(d, allow=bad) == capi.BAD_ARG
        t = torch.from_numpy(d).to("cuda:0")
        torch.cuda.synchronize()
        assert p.add_descriptors_device(t, 1, allow=bad) == capi.BAD_ARG
        unchanged()
    assert p.add(scans[:2], allow=cap) == capi.CAPACITY                       # 3 + 2 > 4: not even the first of the batch
    assert p.add_descriptors(before[:2], allow=cap) == capi.CAPACITY
    unchanged()
    t = torch.from_numpy(before[:1].copy()).to("cuda:0")
    torch.cuda.synchronize()
    assert p.add_descriptors_device(t, 1) == 3 and p.size() == 4              # a good device add still goes through
    assert np.array_equal(p.get(3, 1), before[:1])
    assert p.add(s0, allow=cap) == capi.CAPACITY and p.size() == 4
    for kw in (dict(n_ring=0), dict(n_ring=33), dict(n_sector=0), dict(n_sector=61), dict(n_sector=122), dict(min_range=-0.1),
               dict(min_range=80.0), dict(max_range=float("nan")), dict(height_offset=float("inf")), dict(capacity=0)):
        with pytest.raises(capi.MsflError):
            capi.Places(0, **kw)


# ---- the rest of the library does not notice ----------------------------------------------------------------------------

def test_matcher_is_bit_identical_around_place_calls(gpu, places):
    from tests import common
    _, mc, ms = common.small_world()
    sc = common.scans(2)
    feats = []
    for pts, ring, _, guess in sc:
        f = gpu.extract_features(pts, ring)
        feats.append((gpu.voxel_downsample(f["full"][f["less_sharp"]], 0.2), gpu.voxel_downsample(f["full"][f["less_flat"]], 0.4), guess))
    corner = np.concatenate([f[0] for f in feats])
    surf = np.concatenate([f[1] for f in feats])
    co, so = _offsets([f[0] for f in feats]), _offsets([f[1] for f in feats])
    guesses = np.stack([f[2] for f in feats])
    gpu.set_map(mc, ms)

    def run():
        return [np.asarray(x).tobytes() for x in gpu.match_scan2map_batch(corner, co, surf, so, guesses.copy())[:2]]

    first = run()
    p = places()
    p.add([s[0] for s in sc])
    p.query(sc[0][0], n_prefilter=1, k=2)
    p.query_entries(1, k=2)
    assert run() == first


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------

def test_cpp_place_database_equals_the_ctypes_path(places, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "place_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "place_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    db, qs, k, npre = list(world_scans()[:5]), list(query_scans()[:2]), 3, 4
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(db), len(qs), k, npre], np.int32).tobytes())
        for s in db + qs:
            f.write(np.int32(len(s)).tobytes())
            f.write(np.ascontiguousarray(s, np.float32).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    p = places()
    p.add(db)
    want = p.query(qs, n_prefilter=npre, k=k)
    assert len(raw) == want.nbytes + 8 * len(qs)
    assert raw[:want.nbytes] == want.tobytes()
    yaw = np.frombuffer(raw[want.nbytes:], np.float64)
    assert np.array_equal(yaw, capi.place_yaw(want["shift"][:, 0], 60))
    assert want["index"][:, 0].tolist() == [0, 1] and want["shift"][:, 0].tolist() == [6, 12]
