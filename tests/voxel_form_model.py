"""What decides a cloud's route through the voxel filter's four forms, restated in numpy.

The filter (pcl::VoxelGrid, bit for bit) has four implementations behind msfl_voxel_downsample_batch; a cloud is handed from one to
the next by flags written on the device (msf_loam_amd/csrc/msfl_extract.cuh, voxel_cloud_body; the host side is
msfl_api_stage_ab.inc).  This model computes, for one cloud and one form, everything those hand-overs look at -- it does NOT compute
centroids (the oracle does) -- so that tests/test_voxel_form_model.py can prove that every case of tests/voxel_limit_cases.py sits on
the side of its edge that its name claims.

Every constant is written out here with the line of msfl_extract.cuh it mirrors (`:N`); a change there must be made here too, and
the case table then shows which cases left their edge.
"""
import numpy as np

INT32_MAX = 0x7FFFFFFF

# form -> what it holds.  S = voxel_cloud_lds_kernel<4, 512>, L = <16, 768>, B = voxel_cloud_big_kernel (voxel_cloud_body<16, 4096, true, true>)
FORMS = {
    #            kVoxWaves       kMaxPoints :1271       kVoxMaxRuns :1264   kCB :1268       kFB :1268      kMultiCap, kBigCap :1556                refusal flag :1299, :1415
    "S": dict(waves=4, max_points=4096, max_runs=4 * 512, coord_bits=14, first_bits=16, multi_cap=4 * 240, big_cap=4 * 16, refuse=5),
    "L": dict(waves=16, max_points=65535, max_runs=16 * 768, coord_bits=14, first_bits=16, multi_cap=16 * 240, big_cap=16 * 16, refuse=4),
    "B": dict(waves=16, max_points=131071, max_runs=16 * 4096, coord_bits=13, first_bits=18, multi_cap=16 * 240, big_cap=16 * 16, refuse=4),
}
CHUNK = 64                    # a run never crosses a 64-point chunk: lane 0 always opens one (:1355); 6-bit length field (:1267)
BIG_VOXEL = 512               # MSFL_VOX_BIG_VOXEL (:1552): more LATER points than this and a whole wavefront sums the voxel (:1616)
RADIX_BITS = 8                # the LSD radix sort's digit (:1471)
G_COORD_LIMIT = 1e9           # voxel_batch_desc_kernel: |floor(p * inv_leaf)| < 1e9 or "leaf too small" (:1089)


def max_chunks(form):
    """kMaxChunks (:1285): entries of the chunk table."""
    return FORMS[form]["waves"] * (128 if form == "B" else 64)


def coord_limit(form):
    """Largest |voxel coordinate| the form's record holds: fabsf(f) < kCoordOff - 1 (:1340), kCoordOff = 1 << (kCB - 1) (:1269)."""
    return (1 << (FORMS[form]["coord_bits"] - 1)) - 2


def voxel_coords(cloud, leaf):
    """floorf(p * inv_leaf) per axis as the kernels compute it (f32 product, then floor): (n, 3) float32."""
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor(cloud[:, :3].astype(np.float32) * inv).astype(np.float32)


def slices(n, form):
    """(seg, [(k0, k1)] per wavefront): seg = ((n + W - 1) / W + 63) & ~63, k0 = wave * seg, k1 = min(k0 + seg, n) (:1305-1306); a
    slice with k0 >= k1 is empty.  Every slice starts on a multiple of 64."""
    w = FORMS[form]["waves"]
    seg = ((n + w - 1) // w + 63) & ~63
    return seg, [(i * seg, min(i * seg + seg, n)) for i in range(w)]


def chunk_heads(coords, n):
    """Head flags of the one-workgroup forms (:1355): a point opens a run when it is lane 0 of its chunk (forced) or its voxel
    differs from its predecessor's.  Slices are whole chunks, so the chunk grid is the same in all three forms."""
    head = np.ones(n, bool)
    if n > 1:
        head[1:] = np.any(coords[1:] != coords[:-1], axis=1)
    forced = np.zeros(n, bool)
    forced[::CHUNK] = True
    return head | forced, forced & ~head


def analyse(cloud, leaf):
    """Everything form-independent about one cloud: coordinates, runs, cells, multi-run voxels, later points."""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 4)
    n = len(cloud)
    a = dict(n=n, finite_xyz=bool(np.isfinite(cloud[:, :3]).all()), finite_w=bool(np.isfinite(cloud[:, 3]).all()))
    if n == 0 or not a["finite_xyz"]:
        return a
    f = voxel_coords(cloud, leaf)
    a["coord_abs_max"] = float(np.abs(f).max())
    a["coord_min"] = f.min(axis=0).astype(np.float64)
    a["coord_max"] = f.max(axis=0).astype(np.float64)
    div = [int(a["coord_max"][k]) - int(a["coord_min"][k]) + 1 for k in range(3)]        # python ints: no overflow
    a["div"] = div
    a["cells"] = div[0] * div[1] * div[2]
    nbits = 1
    while (1 << nbits) < a["cells"]:
        nbits += 1                                                                       # :1463-1464
    a["nbits"] = nbits
    a["radix_passes"] = (nbits + RADIX_BITS - 1) // RADIX_BITS
    if a["coord_abs_max"] >= G_COORD_LIMIT:
        return a                                                                         # no form looks further
    c = f.astype(np.int64)
    head, forced = chunk_heads(c, n)
    a["head"] = head
    a["forced_heads"] = int(forced.sum())                     # runs cut by a chunk boundary alone
    a["runs"] = int(head.sum())
    a["runs_g"] = int((head & ~forced).sum())                 # the device-wide form cuts nothing (voxel_batch_head_kernel)
    rel = c - c.min(axis=0)
    cell = rel[:, 0] + rel[:, 1] * div[0] + rel[:, 2] * div[0] * div[1]
    a["cell"] = cell
    starts = np.flatnonzero(head)
    lens = np.diff(np.r_[starts, n])
    a["run_start"], a["run_len"] = starts, lens
    run_cell = cell[starts]
    order = np.argsort(run_cell, kind="stable")               # what the stable sort leaves: a voxel's runs in arrival order
    sc = run_cell[order]
    vstart = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    vruns = np.diff(np.r_[vstart, len(sc)])
    vpoints = np.add.reduceat(lens[order], vstart)
    later = vpoints - lens[order][vstart]
    a["voxels"] = len(vstart)
    a["multi"] = int((vruns > 1).sum())
    a["later"] = later
    a["later_max"] = int(later.max())
    a["n_big"] = int((later > BIG_VOXEL).sum())
    a["voxel_of_run"] = (order, vstart, vruns)
    return a


def verdict(a, form):
    """The flag the form leaves for the cloud (0 served, 1 leaf too small, 3 non-finite, 4 / 5 handed on) and the branches it
    takes when it serves it."""
    F = FORMS[form]
    if a["n"] > F["max_points"]:
        return dict(flag=F["refuse"], why="points")                                     # :1299
    if a["n"] == 0:
        return dict(flag=0, why="empty")
    if not a["finite_xyz"]:
        return dict(flag=3, why="non-finite")                                           # :1339
    flag, why = 0, "served"
    if not (a["coord_abs_max"] <= coord_limit(form)) or not a["finite_w"]:
        flag, why = 4, "coordinates" if a["finite_w"] else "4th field"                  # :1340, :1344
    if a.get("runs", 0) > F["max_runs"]:
        if F["refuse"] > flag:
            why = "runs"
        flag = max(flag, F["refuse"])                                                   # :1415
    if flag == 0 and a["cells"] > INT32_MAX:
        return dict(flag=1, why="cells")                                                # :1420-1422
    if flag:
        return dict(flag=flag, why=why)
    seg, sl = slices(a["n"], form)
    big = a["later"] > BIG_VOXEL
    out = dict(flag=0, why="served", seg=seg, slices=sl, runs=a["runs"], pool_left=F["max_runs"] - a["runs"],
               chunks=sum((k1 - k0 + CHUNK - 1) // CHUNK for k0, k1 in sl if k1 > k0),
               radix_passes=a["radix_passes"], multi=a["multi"],
               multi_overflow=max(a["multi"] - F["multi_cap"], 0),                      # voxels finished in pass 1 after all (:1600-1601)
               n_big=int(big.sum()), big_overflow=max(int(big.sum()) - F["big_cap"], 0),
               wave_walk_rounds=(min(int(big.sum()), F["big_cap"]) + F["waves"] - 1) // F["waves"])    # the q += kVoxWaves loop (:1628)
    assert out["chunks"] <= max_chunks(form)
    return out


def g_verdict(a):
    """voxel_batch_desc_kernel's VoxelCloudDesc::bad (:1085-1095) and what set it: 0, 1 leaf too small (a coordinate no int holds
    :1089, or too many cells :1093), 3 non-finite.  (2, no finite point in a non-empty cloud :1085, never leaves the kernel: such a
    cloud has a non-finite point, and :1095 then writes 3 over it.)"""
    if a["n"] == 0:
        return dict(flag=0, why="empty")
    if not a["finite_xyz"]:
        return dict(flag=3, why="non-finite")
    if a["coord_abs_max"] >= G_COORD_LIMIT:
        return dict(flag=1, why="coordinates")
    if a["cells"] > INT32_MAX:
        return dict(flag=1, why="cells")
    return dict(flag=0, why="served")


def g_key(analyses):
    """The device-wide form's sort key for a batch (msfl_api_stage_ab.inc:549-556): cell, cloud and run-number widths, and whether
    the run number still rides in the key (64 bits at the most) or the sort is a (key, value) one."""
    good = [a for a in analyses if a["n"] > 0 and g_verdict(a)["flag"] == 0]
    max_cells = max([a["cells"] for a in good], default=0)
    runs = sum(a["runs_g"] for a in good)
    bits = lambda x: next(b for b in range(1, 64) if (1 << b) >= x)
    cell_bits, cloud_bits, rid_bits = bits(max_cells), bits(len(analyses)), bits(runs)
    total = cell_bits + cloud_bits + rid_bits
    return dict(cell_bits=cell_bits, cloud_bits=cloud_bits, rid_bits=rid_bits, key_bits=total, pairs_sort=total > 64, runs=runs)


def route_batch(clouds, leaf, handle="default"):
    """Which form delivers each cloud of a batch on a handle ("default", "no_big" = MSFL_VOXEL_NO_BIG, "global" = MSFL_VOXEL_GLOBAL)
    and the status of the call.  Returns dict(status, served=[form or "refused" or "empty"], path=[[(form, flag), ...]], analyses)."""
    an = [analyse(c, leaf) for c in clouds]
    path = [[] for _ in clouds]
    flags = [None] * len(clouds)
    if handle != "global":
        for b, a in enumerate(an):
            v = verdict(a, "S"); path[b].append(("S", v["flag"])); flags[b] = v["flag"]
            if v["flag"] == 5:                                    # only what S escalated is looked at by L (only_escalated == 1)
                v = verdict(a, "L"); path[b].append(("L", v["flag"])); flags[b] = v["flag"]
        if handle == "default" and any(fl == 4 for fl in flags):
            for b, a in enumerate(an):
                if flags[b] == 4:
                    v = verdict(a, "B"); path[b].append(("B", v["flag"])); flags[b] = v["flag"]
    if handle == "global" or any(fl == 4 for fl in flags):         # one refused cloud sends the WHOLE batch to the device-wide form
        for b, a in enumerate(an):
            flags[b] = g_verdict(a)["flag"]; path[b].append(("G", flags[b]))
    served = []
    for b, a in enumerate(an):
        served.append("empty" if a["n"] == 0 else "refused" if flags[b] else path[b][-1][0])
    status = "BAD_ARG" if any(fl in (2, 3) for fl in flags) else "CAPACITY" if any(fl == 1 for fl in flags) else "OK"
    return dict(status=status, served=served, path=path, analyses=an)
