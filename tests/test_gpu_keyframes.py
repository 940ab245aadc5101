"""msfl_keyframes_*: the keyframe store against the oracle's own building blocks (oracle.transform_cloud, oracle.voxel_grid,
oracle.HybridGrid) and against the calls it replaces (Handle.transform_cloud, Handle.voxel_downsample, Grid.insert_scan).  Every
comparison is np.array_equal: both sides run the same stated f32 / f64 operations in the same order.

Keyframe sizes per kind come from SIZES (around the wavefront, the 1 024-point chunk of the gather kernel, and several chunks);
points are uniform in +-30 m with a random t, poses are random with translations up to 50 m."""
import functools

import numpy as np
import pytest

from tests import common
from tests import windowed_grid_model as wm

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097)
SENTINEL = np.float32(-12345.5)


def _cloud(rng, n):
    return np.ascontiguousarray(np.c_[rng.uniform(-30, 30, (n, 3)), rng.uniform(0, 0.1, n)].astype(np.float32))


def _poses(rng, n, reach=50.0):
    q = rng.normal(0, 1, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(np.c_[rng.uniform(-reach, reach, (n, 3)), q])


@functools.lru_cache(maxsize=None)
def _lists():
    """Nine keyframes; keyframe i has SIZES[i] corner points and SIZES[(4 i + 3) % 9] surf points (every size once per kind; key 8
    has 4 097 of both)."""
    rng = np.random.default_rng(2024)
    return [(_cloud(rng, SIZES[i]), _cloud(rng, SIZES[(4 * i + 3) % 9])) for i in range(9)]


@pytest.fixture(scope="module")
def store(gpu):
    """The nine keyframes stored as given (both leaves 0)."""
    from msf_loam_amd import capi
    k = capi.Keyframes(gpu, max_keyframes=64, max_corner_points=1 << 15, max_surf_points=1 << 15, leaf_corner=0.0, leaf_surf=0.0)
    for i, (c, s) in enumerate(_lists()):
        assert k.add(c, s) == i
    yield k
    k.close()


def _cat(parts):
    parts = [p for p in parts]
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def _expect(oracle, member_off, keys, poses, kind):
    """Per submap the concatenation of oracle.transform_cloud outputs, member order."""
    out = []
    for b in range(len(member_off) - 1):
        out.append(_cat([np.zeros((0, 4), np.float32)] +
                        [oracle.transform_cloud(_lists()[keys[m]][kind], poses[m]) for m in range(member_off[b], member_off[b + 1])
                         if len(_lists()[keys[m]][kind])]))
    return out


def _split(pts, off):
    return [pts[off[b]:off[b + 1]] for b in range(len(off) - 1)]


# ---- 1. add / get / sizes --------------------------------------------------------------------------------------------------

def test_add_get_sizes_round_trip_bytes_host_device_and_index_lists(gpu, store):
    import torch
    from msf_loam_amd import capi
    nc, ns = store.sizes()
    assert nc.tolist() == [len(c) for c, _ in _lists()] and ns.tolist() == [len(s) for _, s in _lists()]
    assert store.size() == len(store) == 9
    for i, (c, s) in enumerate(_lists()):
        gc, gs = store.get(i)
        assert gc.tobytes() == c.tobytes() and gs.tobytes() == s.tobytes(), i
    assert store.sizes(3, 2)[0].tolist() == [SIZES[3], SIZES[4]]
    # device memory, the array itself and the index-list form (one full cloud, two lists into it: the shape of Slam.clouds())
    rng = np.random.default_rng(5)
    k = capi.Keyframes(gpu, max_keyframes=8, max_corner_points=8192, max_surf_points=8192, leaf_corner=0.0, leaf_surf=0.0)
    full = _cloud(rng, 5000)
    full[7, 2] = -0.0                                     # bytes, not values
    ci = rng.permutation(5000)[:1025].astype(np.int32)
    si = rng.permutation(5000)[:2049].astype(np.int32)
    d_full, d_ci, d_si = torch.from_numpy(full).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(si).cuda()
    torch.cuda.synchronize()
    assert k.add_device(d_full, 5000, d_full, 63) == 0
    assert k.add_device(d_full, len(ci), d_full, len(si), corner_idx=d_ci, surf_idx=d_si) == 1
    assert k.add(full, full, corner_idx=ci, surf_idx=si) == 2
    assert k.add(full[:0], full[:1]) == 3
    want = [(full, full[:63]), (full[ci], full[si]), (full[ci], full[si]), (full[:0], full[:1])]
    for i, (c, s) in enumerate(want):
        gc, gs = k.get(i)
        assert gc.tobytes() == c.tobytes() and gs.tobytes() == s.tobytes(), i
    d_c, d_s = torch.zeros((1025, 4), device="cuda"), torch.zeros((2049, 4), device="cuda")
    torch.cuda.synchronize()
    k.get_device(1, d_c, 1025, d_s, 2049)
    gpu.synchronize()
    assert np.array_equal(d_c.cpu().numpy(), full[ci]) and np.array_equal(d_s.cpu().numpy(), full[si])
    with pytest.raises(capi.MsflError) as e:
        k.get_device(1, d_c, 1024, d_s, 2049)
    assert e.value.status == capi.CAPACITY
    k.close()


@pytest.mark.parametrize("form", ("host", "device", "device_idx"))
def test_add_with_leaves_stores_what_the_voxel_filter_returns(gpu, oracle, form):
    import torch
    from msf_loam_amd import capi
    rng = np.random.default_rng(6)
    k = capi.Keyframes(gpu, max_keyframes=16, max_corner_points=1 << 16, max_surf_points=1 << 16, leaf_corner=0.2, leaf_surf=0.4)
    for n_c, n_s in ((1025, 4097), (0, 65), (64, 0), (4097, 1023)):
        # a dense box: several points per voxel, so the filter has something to average
        full = np.ascontiguousarray(np.c_[rng.uniform(-3, 3, (6000, 3)), rng.uniform(0, 0.1, 6000)].astype(np.float32))
        ci, si = rng.permutation(6000)[:n_c].astype(np.int32), rng.permutation(6000)[:n_s].astype(np.int32)
        c, s = full[ci], full[si]
        if form == "host":
            i = k.add(c, s)
        elif form == "device":
            d_c, d_s = torch.from_numpy(np.ascontiguousarray(c)).cuda(), torch.from_numpy(np.ascontiguousarray(s)).cuda()
            torch.cuda.synchronize()
            i = k.add_device(d_c, n_c, d_s, n_s)
        else:
            d_full, d_ci, d_si = torch.from_numpy(full).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(si).cuda()
            torch.cuda.synchronize()
            i = k.add_device(d_full, n_c, d_full, n_s, corner_idx=d_ci, surf_idx=d_si)
        gc, gs = k.get(i)
        for got, pts, leaf in ((gc, c, 0.2), (gs, s, 0.4)):
            assert np.array_equal(got, gpu.voxel_downsample(pts, leaf)) and np.array_equal(got, oracle.voxel_grid(pts, leaf))
            assert len(got) <= len(pts) and (len(pts) < 1023 or len(got) < len(pts))      # the filter had something to average
        assert (k.sizes(i, 1)[0][0], k.sizes(i, 1)[1][0]) == (len(gc), len(gs))
    k.close()


def test_add_refusals_leave_the_store_unchanged(gpu):
    import torch
    from msf_loam_amd import capi
    rng = np.random.default_rng(7)
    c0, s0 = _cloud(rng, 60), _cloud(rng, 30)
    for leaves in ((0.0, 0.0), (0.2, 0.4)):
        k = capi.Keyframes(gpu, max_keyframes=4, max_corner_points=4096, max_surf_points=4096, leaf_corner=leaves[0], leaf_surf=leaves[1])
        assert k.add(c0, s0) == 0
        before = [a.tobytes() for a in k.get(0)]
        for bad in (np.nan, np.inf, -np.inf):
            for coord in range(4):
                for kind in range(2):
                    lists = [_cloud(rng, 1025), _cloud(rng, 65)]
                    lists[kind][len(lists[kind]) // 2, coord] = bad
                    assert k.add(lists[0], lists[1], allow=(capi.BAD_ARG,)) == capi.BAD_ARG
                    d = [torch.from_numpy(a).cuda() for a in lists]
                    torch.cuda.synchronize()
                    assert k.add_device(d[0], 1025, d[1], 65, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
                    assert k.size() == 1
        assert [a.tobytes() for a in k.get(0)] == before
        assert k.add(c0, s0) == 1 and np.array_equal(k.get(1)[0], k.get(0)[0])        # and the store still works
        k.close()
    # pools and the keyframe count, one past capacity
    k = capi.Keyframes(gpu, max_keyframes=2, max_corner_points=100, max_surf_points=50, leaf_corner=0.0, leaf_surf=0.0)
    assert k.add(c0, s0) == 0
    before = [a.tobytes() for a in k.get(0)]
    assert k.add(_cloud(rng, 41), _cloud(rng, 0), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert k.add(_cloud(rng, 40), _cloud(rng, 21), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert k.size() == 1 and [a.tobytes() for a in k.get(0)] == before
    assert k.add(_cloud(rng, 40), _cloud(rng, 20)) == 1
    assert k.add(_cloud(rng, 0), _cloud(rng, 0), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert k.size() == 2 and [a.tobytes() for a in k.get(0)] == before and k.sizes()[0].tolist() == [60, 40]
    with pytest.raises(capi.MsflError) as e:
        k.add(_cloud(rng, 1), _cloud(rng, 1))
    assert e.value.status == capi.CAPACITY
    k.close()


# ---- 2. / 3. compose -------------------------------------------------------------------------------------------------------

def _case(B):
    """Members over all nine keyframes.  B = 5: key 6 twice inside submap 0, key 8 in submaps 0, 1 and 4, key 0 (no corner
    points) and key 6 (no surf points) as members, submap 2 without members, member_off[0] = 2."""
    rng = np.random.default_rng(40 + B)
    if B == 1:
        keys = np.array([99, -1, 3, 0, 6, 3, 8, 1], np.int32)           # positions 0, 1 are never read
        member_off = np.array([2, 8], np.int32)
    else:
        keys = np.array([77, 77, 6, 8, 6, 0, 5, 8, 2, 7, 1, 3, 4, 8, 0], np.int32)
        member_off = np.array([2, 6, 9, 9, 12, 15], np.int32)
    poses = _poses(rng, len(keys))
    poses[:2] = np.nan                                                  # never read either
    return member_off, keys, poses


@pytest.mark.parametrize("B", (1, 5))
def test_compose_leaf_zero_is_the_concatenation_of_transformed_keyframes(gpu, oracle, store, B):
    member_off, keys, poses = _case(B)
    assert SIZES[(4 * 6 + 3) % 9] == 0 and 6 in keys and 0 in keys       # a member of size 0 in either kind
    corner, off_c, surf, off_s = store.compose(member_off, keys, poses)
    assert off_c[0] == 0 and off_s[0] == 0
    for kind, (pts, off) in enumerate(((corner, off_c), (surf, off_s))):
        want = _expect(oracle, member_off, keys, poses, kind)
        assert off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        for b, (got, w) in enumerate(zip(_split(pts, off), want)):
            assert np.array_equal(got, w), (kind, b)
            mine = _cat([np.zeros((0, 4), np.float32)] + [gpu.transform_cloud(_lists()[keys[m]][kind], poses[m])
                                                         for m in range(member_off[b], member_off[b + 1]) if len(_lists()[keys[m]][kind])])
            assert np.array_equal(got, mine), (kind, b)
    if B == 5:
        assert off_c[3] == off_c[2] and off_s[3] == off_s[2]            # the submap without members


def test_compose_with_leaves_is_the_voxel_filter_of_the_concatenation(gpu, oracle, store):
    member_off, keys, poses = _case(5)
    corner, off_c, surf, off_s = store.compose(member_off, keys, poses, 0.2, 0.4)
    for kind, (pts, off, leaf) in enumerate(((corner, off_c, 0.2), (surf, off_s, 0.4))):
        want = [oracle.voxel_grid(w, leaf) for w in _expect(oracle, member_off, keys, poses, kind)]
        assert off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        for b, (got, w) in enumerate(zip(_split(pts, off), want)):
            assert np.array_equal(got, w), (kind, b)
    # the B = 5 call equals five B = 1 calls; and a leaf on one kind only
    for b in range(5):
        c1, oc1, s1, os1 = store.compose(member_off[b:b + 2], keys, poses, 0.2, 0.4)
        assert np.array_equal(c1, corner[off_c[b]:off_c[b + 1]]) and np.array_equal(s1, surf[off_s[b]:off_s[b + 1]])
        assert oc1.tolist() == [0, off_c[b + 1] - off_c[b]] and os1.tolist() == [0, off_s[b + 1] - off_s[b]]
    c0, oc0, s4, os4 = store.compose(member_off, keys, poses, 0.0, 0.4)
    assert np.array_equal(s4, surf) and np.array_equal(c0, _cat(_expect(oracle, member_off, keys, poses, 0)))


# ---- 4. the large voxel forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_members", (17, 40))
def test_compose_one_large_submap_takes_the_big_voxel_forms(oracle, store, n_members):
    """17 x 4 097 = 69 649 points per kind (above 65 535: the big one-workgroup form or the device-wide one) and 40 x 4 097 =
    163 880 (above 131 071: the device-wide form), key 8 at n_members poses."""
    rng = np.random.default_rng(50 + n_members)
    keys = np.full(n_members, 8, np.int32)
    poses = _poses(rng, n_members, 20.0)
    member_off = np.array([0, n_members], np.int32)
    assert store.member_totals(member_off, keys) == (n_members * 4097, n_members * 4097)
    corner, off_c, surf, off_s = store.compose(member_off, keys, poses, 0.2, 0.4)
    for kind, (pts, leaf) in enumerate(((corner, 0.2), (surf, 0.4))):
        want = oracle.voxel_grid(_expect(oracle, member_off, keys, poses, kind)[0], leaf)
        assert np.array_equal(pts, want), kind


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------

def test_compose_refusals_launch_nothing_and_write_nothing(gpu, store):
    from msf_loam_amd import capi
    member_off, keys, poses = _case(5)
    tc, ts = store.member_totals(member_off, keys)

    def refused(status, member_off=member_off, keys=keys, poses=poses, leaf_corner=0.0, leaf_surf=0.0, short=(0, 0)):
        oc, os_ = np.full((tc, 4), SENTINEL), np.full((ts, 4), SENTINEL)
        s = store.compose(member_off, keys, poses, leaf_corner, leaf_surf, allow=(status,), out_corner=oc, out_surf=os_,
                          cap_corner=tc - short[0], cap_surf=ts - short[1])
        assert s == status, s
        gpu.synchronize()
        assert (oc == SENTINEL).all() and (os_ == SENTINEL).all()

    for bad_key in (9, -1, 1 << 30):
        k2 = keys.copy(); k2[7] = bad_key
        refused(capi.BAD_ARG, keys=k2)
    for bad in (np.nan, np.inf, -np.inf):
        for entry in (0, 3, 6):
            p2 = poses.copy(); p2[9, entry] = bad
            refused(capi.BAD_ARG, poses=p2)
    refused(capi.BAD_ARG, member_off=np.array([2, 6, 5, 9, 12, 15], np.int32))
    for leaf in (np.nan, -0.2, np.inf):
        refused(capi.BAD_ARG, leaf_corner=leaf)
        refused(capi.BAD_ARG, leaf_surf=leaf)
    refused(capi.CAPACITY, short=(1, 0))
    refused(capi.CAPACITY, short=(0, 1))
    refused(capi.CAPACITY, short=(1, 0), leaf_corner=0.2, leaf_surf=0.4)
    # and the unrefused call still works afterwards
    assert len(store.compose(member_off, keys, poses)[0]) == tc


# ---- 6. device-resident hand-over ------------------------------------------------------------------------------------------

def test_compose_device_feeds_match_pairs_batch_device(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    sc = common.scans(4)
    feats = [common.features_from_oracle(oracle, pts, ring)[1:] for pts, ring, _, _ in sc]
    k = capi.Keyframes(gpu, max_keyframes=8, max_corner_points=1 << 16, max_surf_points=1 << 17, leaf_corner=0.0, leaf_surf=0.0)
    for c, s in feats:
        k.add(c, s)
    tiny = k.add(feats[0][0][:3], feats[0][1][:50])                         # fewer than 5 corner points
    # pair p: scan p against the submap of the other three scans laid down in the world frame; pair 3: against the tiny keyframe
    keys = np.array([1, 2, 3, 0, 2, 3, 0, 1, 3, tiny], np.int32)
    member_off = np.array([0, 3, 6, 9, 10], np.int32)
    poses = np.array([sc[j][2] for j in keys[:9]] + [sc[0][2]])
    P = 4
    tc, ts = k.member_totals(member_off, keys)
    d_mc, d_ms = torch.zeros((tc, 4), device="cuda"), torch.zeros((ts, 4), device="cuda")
    corner = np.concatenate([feats[p][0] for p in range(P)]); co = np.cumsum([0] + [len(feats[p][0]) for p in range(P)]).astype(np.int32)
    surf = np.concatenate([feats[p][1] for p in range(P)]); so = np.cumsum([0] + [len(feats[p][1]) for p in range(P)]).astype(np.int32)
    guesses = np.array([sc[p][3] for p in range(P)])
    d_c, d_s = torch.from_numpy(corner).cuda(), torch.from_numpy(surf).cuda()
    d_poses, d_status = torch.from_numpy(guesses.copy()).cuda(), torch.full((P,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for leaves in ((0.0, 0.0), (0.2, 0.4)):
        d_poses.copy_(torch.from_numpy(guesses)); d_status.fill_(-1)
        torch.cuda.synchronize()
        mco, mso = k.compose_device(member_off, keys, poses, leaves[0], leaves[1], d_mc, tc, d_ms, ts)
        gpu.match_pairs_batch_device(P, d_mc, mco, d_ms, mso, d_c, co, d_s, so, d_poses, d_status)
        gpu.synchronize()
        got_poses, got_status = d_poses.cpu().numpy(), d_status.cpu().numpy()
        mc, ms = d_mc.cpu().numpy()[:mco[-1]], d_ms.cpu().numpy()[:mso[-1]]
        hc, hco, hs, hso = k.compose(member_off, keys, poses, leaves[0], leaves[1])
        assert np.array_equal(mc, hc) and np.array_equal(ms, hs) and mco.tolist() == hco.tolist() and mso.tolist() == hso.tolist()
        want_poses, want_status, _ = gpu.match_pairs_batch(mc, mco, ms, mso, corner, co, surf, so, guesses)
        assert np.array_equal(got_poses, want_poses) and np.array_equal(got_status, want_status)
        assert got_status.tolist() == [0, 0, 0, capi.MAP_TOO_SMALL] and np.array_equal(got_poses[3], guesses[3])
    k.close()


# ---- 7. insert -------------------------------------------------------------------------------------------------------------

def _same_grid(g, m, what):
    assert g.size() == m.size(), what
    assert np.array_equal(g.dump(), m.dump()) and np.array_equal(g.dump_cells(), m.dump_cells()), what


def test_insert_equals_the_loop_of_transform_and_insert_scan(gpu, oracle, store):
    from msf_loam_amd import capi
    rng = np.random.default_rng(70)
    keys = np.array([3, 8, 0, 6, 8, 5, 1, 7], np.int32)
    poses = _poses(rng, len(keys))
    gc, gs = capi.Grid(gpu, 3.0, 0.2), capi.Grid(gpu, 3.0, 0.4)
    lc, ls = capi.Grid(gpu, 3.0, 0.2), capi.Grid(gpu, 3.0, 0.4)
    mc, ms = wm.WindowedGrid(oracle, 3.0, 0.2), wm.WindowedGrid(oracle, 3.0, 0.4)

    def loop(first, last):
        for i in range(first, last):
            c, s = _lists()[keys[i]]
            lc.insert_scan(gpu.transform_cloud(c, poses[i])); ls.insert_scan(gpu.transform_cloud(s, poses[i]))
            mc.insert_scan(oracle.transform_cloud(c, poses[i])); ms.insert_scan(oracle.transform_cloud(s, poses[i]))

    assert store.insert(keys[:5], poses[:5], gc, gs) == (capi.OK, 5)
    loop(0, 5)
    for g, l, m in ((gc, lc, mc), (gs, ls, ms)):
        _same_grid(g, l, "loop"); _same_grid(g, m, "oracle")
    # a keyframe posed 30 000 m out (beyond +-8192 cells of 3 m) ends the call at its position
    far = poses[5:].copy()
    far[1, :3] = (30000.0, 0.0, 0.0)
    assert store.insert(keys[5:], far, gc, gs, allow=(capi.CAPACITY,)) == (capi.CAPACITY, 1)
    loop(5, 6)
    for g, l, m in ((gc, lc, mc), (gs, ls, ms)):
        _same_grid(g, l, "loop after the refusal"); _same_grid(g, m, "oracle after the refusal")
    # one store only; and the call goes on working
    assert store.insert(keys[6:], poses[6:], None, gs) == (capi.OK, 2)
    for i in (6, 7):
        ls.insert_scan(gpu.transform_cloud(_lists()[keys[i]][1], poses[i]))
    _same_grid(gs, ls, "surf only"); _same_grid(gc, lc, "corner untouched")
    # refusals that insert nothing
    before = gc.dump().tobytes()
    other = capi.Handle(0)
    og = capi.Grid(other, 3.0, 0.2)
    assert store.insert(keys[:2], poses[:2], og, gs, allow=(capi.BAD_ARG,)) == (capi.BAD_ARG, 0)
    assert store.insert(keys[:2], poses[:2], gc, og, allow=(capi.BAD_ARG,)) == (capi.BAD_ARG, 0)
    assert og.size() == (0, 0)
    og.close(); other.close()
    bad_pose = poses[:2].copy(); bad_pose[1, 4] = np.nan
    assert store.insert(keys[:2], bad_pose, gc, gs, allow=(capi.BAD_ARG,)) == (capi.BAD_ARG, 0)
    assert store.insert(np.array([1, 9], np.int32), poses[:2], gc, gs, allow=(capi.BAD_ARG,)) == (capi.BAD_ARG, 0)
    assert gc.dump().tobytes() == before
    for g in (gc, gs, lc, ls):
        g.close()


def test_unfiltered_keyframes_inserted_at_the_session_poses_rebuild_the_session_map(gpu):
    """A SLAM session inserts every scan's whole less-sharp / less-flat list at pose_map.  A store with both leaves 0 fed those
    lists (Slam.clouds(): full_scan with the two index lists), inserted at the session's own pose_map, is the session's map."""
    from msf_loam_amd import capi, synth
    n = 8
    world = common.small_world()[0]
    truth = [np.r_[0.4 * k, 0.05 * k, 1.8, synth.quat_from_euler(0.0, 0.0, 0.02 * k)] for k in range(n)]
    scans = [synth.make_scan(world, truth[k], synth.SEED + 900 + k) for k in range(n)]
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans), max_rings=16, pose_odom2map=truth[0], keep_clouds=1)
    k0 = capi.Keyframes(gpu, max_keyframes=n, max_corner_points=1 << 17, max_surf_points=1 << 19, leaf_corner=0.0, leaf_surf=0.0)
    pose_map = []
    for k, (pts, ring) in enumerate(scans):
        r = slam.add_scan(pts, ring)
        assert r.status_extract == 0 and r.status_insert == 0
        pose_map.append(np.array(r.pose_map[:]))
        cl = slam.clouds(k)
        assert k0.add(cl["full_scan"], cl["full_scan"], corner_idx=cl["less_sharp"], surf_idx=cl["less_flat"]) == k
    sc, ss = slam.grids()
    gc, gs = capi.Grid(gpu, 3.0, 0.2), capi.Grid(gpu, 3.0, 0.4)
    assert k0.insert(np.arange(n), pose_map, gc, gs) == (capi.OK, n)
    for mine, session in ((gc, sc), (gs, ss)):
        assert mine.size() == session.size() and mine.size()[0] > 0
        assert np.array_equal(mine.dump(), session.dump()) and np.array_equal(mine.dump_cells(), session.dump_cells())
    gc.close(); gs.close(); k0.close(); slam.close()


# ---- 8. isolation ----------------------------------------------------------------------------------------------------------

def test_a_matcher_call_after_the_store_is_bit_identical_to_a_fresh_handle(oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    pts, ring, _, guess = common.scans(1)[0]
    _, c, s = common.features_from_oracle(oracle, pts, ring)
    fresh = capi.Handle(0)
    fresh.set_map(mc, ms)
    st0, pose0, info0 = fresh.match_scan2map(c, s, guess)
    fresh.close()
    h = capi.Handle(0)
    h.set_map(mc, ms)
    k = capi.Keyframes(h, max_keyframes=8, max_corner_points=1 << 15, max_surf_points=1 << 15)
    for _ in range(3):
        k.add(c, s)
    rng = np.random.default_rng(80)
    k.compose([0, 2, 3], [0, 1, 2], _poses(rng, 3), 0.2, 0.4)
    k.compose([0, 3], [0, 1, 2], _poses(rng, 3))
    gc, gs = capi.Grid(h, 3.0, 0.2), capi.Grid(h, 3.0, 0.4)
    assert k.insert([0, 1], _poses(rng, 2), gc, gs) == (capi.OK, 2)
    st1, pose1, info1 = h.match_scan2map(c, s, guess)
    assert st1 == st0 == 0 and pose1.tobytes() == pose0.tobytes()
    assert bytes(info1) == bytes(info0)
    h.close()
