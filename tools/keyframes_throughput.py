"""Throughput of msfl_keyframes_compose against the loop it replaces, of its gather kernel alone, and of msfl_keyframes_insert.
    python tools/keyframes_throughput.py [--submaps 64] [--half-width 10] [--corner 1500] [--surf 5000] [--out profiles/keyframes.json]

  shape      --submaps submaps x (2 x half-width + 1) members; keyframes of about --corner corner and --surf surf points (poles and a
             ground plane with walls, so that the voxel filter has something to merge), on a path of 0.4 m steps; submap b = the
             keyframes j-w .. j+w in j's frame
  compose    one msfl_keyframes_compose with leaves 0.2 / 0.4 into device buffers
  loop       what a caller does without it, same build, public API, device resident: one msfl_transform_cloud per member and kind
             into a concatenated buffer (region b = [corner | surf] of submap b), then msfl_voxel_downsample_batch_pair over it
  gather     compose with both leaves 0 (the gather kernel and its table upload alone, asynchronous), timed with HIP events over
             back-to-back calls; the rate is against 32 algorithmic bytes per point (16 read, 16 written)
  insert     msfl_keyframes_insert of --insert keyframes into two fresh map stores: wall time per keyframe (K existing inserts)

The two legs alternate in one session; the figures are the median of --reps after a warm-up.  Writes one JSON record."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from msf_loam_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--submaps", type=int, default=64)
ap.add_argument("--half-width", type=int, default=10)
ap.add_argument("--corner", type=int, default=1500)
ap.add_argument("--surf", type=int, default=5000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--insert", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframes.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("keyframes_throughput.py needs a GPU (no CPU fallback)")
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
rng = np.random.default_rng(7)
w = args.half_width
n_kf = args.submaps + 2 * w


def keyframe(k):
    """Scan-frame features of a sensor at x = 0.4 k on a 60 m square floor with walls and poles (sizes vary by +-10 %)."""
    n_c, n_s = (int(n * rng.uniform(0.9, 1.1)) for n in (args.corner, args.surf))
    x0 = 0.4 * k
    poles = rng.integers(0, 40, n_c)
    corner = np.c_[(poles % 8) * 7.0 - 25.0 - x0 + rng.normal(0, 0.01, n_c), (poles // 8) * 10.0 - 20.0 + rng.normal(0, 0.01, n_c), rng.uniform(0, 3, n_c)]
    surf = np.c_[rng.uniform(-30, 30, n_s) - x0, rng.uniform(-30, 30, n_s), rng.normal(0, 0.01, n_s)]
    wall = rng.uniform(size=n_s) < 0.3
    surf[wall, 1], surf[wall, 2] = 30.0 + rng.normal(0, 0.01, int(wall.sum())), rng.uniform(0, 3, int(wall.sum()))
    t = lambda n: rng.uniform(0, 0.1, n)
    return (np.ascontiguousarray(np.c_[corner, t(n_c)].astype(np.float32)), np.ascontiguousarray(np.c_[surf, t(n_s)].astype(np.float32)))


lists = [keyframe(k) for k in range(n_kf)]
path = np.array([[0.4 * k, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] for k in range(n_kf)])
h = capi.Handle(0)
stream = torch.cuda.current_stream(dev)
h.set_stream(stream.cuda_stream)
kf = capi.Keyframes(h, max_keyframes=n_kf, max_corner_points=sum(len(c) for c, _ in lists), max_surf_points=sum(len(s) for _, s in lists),
                    leaf_corner=0.0, leaf_surf=0.0)
for c, s in lists:
    kf.add(c, s)
keys, member_off, poses = [], [0], []
for b in range(args.submaps):
    j = b + w
    for i in range(j - w, j + w + 1):
        keys.append(i)
        poses.append(capi.relative_pose(path[j], path[i]))
    member_off.append(len(keys))
keys, member_off, poses = np.array(keys, np.int32), np.array(member_off, np.int32), np.array(poses)
M, B = len(keys), args.submaps
tc, ts = kf.member_totals(member_off, keys)
d_out_c, d_out_s = torch.zeros((tc, 4), device=dev), torch.zeros((ts, 4), device=dev)

# ---- the loop's side: the keyframes as the caller's own device arrays, the concatenated buffer and its index lists ----
d_lists = [(torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev)) for c, s in lists]
nc = np.array([sum(len(lists[i][0]) for i in keys[member_off[b]:member_off[b + 1]]) for b in range(B)])
ns = np.array([sum(len(lists[i][1]) for i in keys[member_off[b]:member_off[b + 1]]) for b in range(B)])
off = np.concatenate([[0], np.cumsum(nc + ns)]).astype(np.int32)
idx_a, idx_b = np.zeros(off[-1], np.int32), np.zeros(off[-1], np.int32)
for b in range(B):
    idx_a[off[b]:off[b] + nc[b]] = np.arange(nc[b])
    idx_b[off[b]:off[b] + ns[b]] = nc[b] + np.arange(ns[b])
d_cat = torch.zeros((int(off[-1]), 4), device=dev)
d_idx_a, d_idx_b = torch.from_numpy(idx_a).to(dev), torch.from_numpy(idx_b).to(dev)
d_cnt_a, d_cnt_b = torch.from_numpy(nc.astype(np.int32)).to(dev), torch.from_numpy(ns.astype(np.int32)).to(dev)
d_loop_c, d_loop_s = torch.zeros((int(off[-1]), 4), device=dev), torch.zeros((int(off[-1]), 4), device=dev)
loop_off_c, loop_off_s = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)
pose_rows = [np.ascontiguousarray(p) for p in poses]
torch.cuda.synchronize(dev)
lib = h.lib


def leg_compose():
    return kf.compose_device(member_off, keys, poses, 0.2, 0.4, d_out_c, tc, d_out_s, ts)


def leg_loop():
    base = d_cat.data_ptr()
    for b in range(B):
        at_c, at_s = int(off[b]), int(off[b]) + int(nc[b])
        for m in range(member_off[b], member_off[b + 1]):
            c, s = d_lists[keys[m]]
            h._check(lib.msfl_transform_cloud(h.h, capi._vp(c), C.c_int(len(c)), capi._vp(pose_rows[m]), C.c_void_p(base + 16 * at_c), C.c_int(capi.MEM_DEVICE)),
                     "msfl_transform_cloud")
            h._check(lib.msfl_transform_cloud(h.h, capi._vp(s), C.c_int(len(s)), capi._vp(pose_rows[m]), C.c_void_p(base + 16 * at_s), C.c_int(capi.MEM_DEVICE)),
                     "msfl_transform_cloud")
            at_c += len(c); at_s += len(s)
    h._check(lib.msfl_voxel_downsample_batch_pair(h.h, C.c_int(B), capi._vp(d_cat), capi._vp(off), capi._vp(d_idx_a), capi._vp(d_cnt_a), C.c_float(0.2),
                                                  capi._vp(d_loop_c), capi._vp(loop_off_c), capi._vp(d_idx_b), capi._vp(d_cnt_b), C.c_float(0.4),
                                                  capi._vp(d_loop_s), capi._vp(loop_off_s), C.c_int(capi.MEM_DEVICE)), "msfl_voxel_downsample_batch_pair")


def wall(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


for _ in range(2):                                      # warm-up of both legs: allocations, the clock ramp
    leg_compose(); leg_loop()
t_compose, t_loop = [], []
for _ in range(args.reps):                              # alternating
    t_compose.append(wall(leg_compose))
    t_loop.append(wall(leg_loop))
off_c, off_s = leg_compose()
leg_loop()
same = bool(np.array_equal(off_c, loop_off_c) and np.array_equal(off_s, loop_off_s) and
            torch.equal(d_out_c[:off_c[-1]], d_loop_c[:off_c[-1]]) and torch.equal(d_out_s[:off_s[-1]], d_loop_s[:off_s[-1]]))

# ---- the gather kernel alone ----
a, b_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(20):
    kf.compose_device(member_off, keys, poses, 0.0, 0.0, d_out_c, tc, d_out_s, ts)
reps = 50
a.record(stream)
for _ in range(reps):
    kf.compose_device(member_off, keys, poses, 0.0, 0.0, d_out_c, tc, d_out_s, ts)
b_ev.record(stream)
torch.cuda.synchronize(dev)
ms_gather = a.elapsed_time(b_ev) / reps

# ---- insert ----
n_ins = min(args.insert, n_kf)
gc, gs = capi.Grid(h, 3.0, 0.2), capi.Grid(h, 3.0, 0.4)
kf.insert(np.arange(2), path[:2], gc, gs)               # warm-up: the stores' first allocations
ms_insert = wall(lambda: kf.insert(np.arange(2, n_ins), path[2:n_ins], gc, gs)) / max(n_ins - 2, 1)

out = {"submaps": B, "members": M, "members_per_submap": 2 * w + 1, "keyframes": n_kf, "points_corner": tc, "points_surf": ts,
       "points_out_corner": int(off_c[-1]), "points_out_surf": int(off_s[-1]),
       "compose_ms": float(np.median(t_compose)), "compose_ms_all": t_compose, "loop_ms": float(np.median(t_loop)), "loop_ms_all": t_loop,
       "loop_over_compose": float(np.median(t_loop) / np.median(t_compose)), "loop_launches_replaced": 2 * M, "legs_bit_identical": same,
       "gather_ms_per_call": ms_gather, "gather_GBps_at_32B_per_point": 32.0 * (tc + ts) / (1e-3 * ms_gather) / 1e9,
       "insert_ms_per_keyframe": ms_insert, "insert_keyframes": n_ins - 2}
gc.close(); gs.close(); kf.close(); h.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
