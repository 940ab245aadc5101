"""CPU: every case of tests/extract_limit_cases.py sits where its name claims.

The extraction computes the same bits on every path, so a case that drifts off its edge (a sector of 511 points, a wrap one point
early, a tie that is none) would still pass its GPU test, on another path.  Here the oracle and plain arithmetic prove each figure:
sector sizes from the sector formula, wrap indices from the oracle's times, tie pairs from the oracle's curvature bits and lists,
seam picks from its labels and lists, list totals and n_full exactly.  The constants those figures rest on are read out of the
kernel source.  The GPU counterpart is tests/test_gpu_extract_limits.py.
"""
import pathlib
import re

import numpy as np
import pytest

from tests import extract_limit_cases as ec

ALL = ec.NAMES + [ec.REFUSED_BATCH]


def _group(prefix):
    return [n for n in ec.NAMES if n.split("_")[0] in prefix]


def _ring_offsets(f):
    """Output offset of every ring id of an oracle result."""
    return np.searchsorted(f["ring"], np.arange(129))


def test_the_table_is_deterministic_and_on_the_lattice():
    assert len(set(ALL)) == len(ALL)
    for name in ALL:
        for pts, ring in ec.case(name).clouds:
            assert pts.dtype == np.float32 and ring.dtype == np.uint16 and len(pts) == len(ring)
            xyz = pts[:, :3][np.isfinite(pts[:, :3])].astype(np.float64)
            assert np.all(xyz * 16 == np.round(xyz * 16)) and np.all(np.abs(xyz) < 1024), name
    for name in ("slices_65", "wrap_256", "tie_3084_7_s4", "seam_last_3084"):
        a = [(p.copy(), r.copy()) for p, r in ec.case(name).clouds]
        ec.case.cache_clear()
        for (p, r), (q, s) in zip(a, ec.case(name).clouds):
            assert np.array_equal(p.view(np.uint32), q.view(np.uint32)) and np.array_equal(r, s)


def test_the_figures_are_the_kernels_constants():
    """The limits the cases straddle, read out of the source text: a limit moved in the kernel alone fails here, where the GPU test
    would pass on the other path.  Nothing is compiled: this pins what is written there."""
    csrc = pathlib.Path(__file__).resolve().parent.parent / "msf_loam_amd" / "csrc"
    squeeze = lambda t: re.sub(r"\s+", "", t)
    cuh, host = squeeze((csrc / "msfl_extract.cuh").read_text()), squeeze((csrc / "msfl_api_stage_ab.inc").read_text())
    assert "constexprintkMaxRings=128;" in cuh
    assert "constexprintkRingCapacity=%d;" % ec.RING_CAPACITY in cuh and "if(len>kRingCapacity){" in cuh
    assert "constexprintkPickCand=8;" in cuh and "constexprintkPickSector=64*kPickCand;" in cuh and ec.PICK_SECTOR == 64 * 8
    assert "constboolin_lds=cnt<=kPickSector;" in cuh
    assert "constintstart=s+5,end=s+len-6;" in cuh and "(end-start>=6)" in cuh
    assert "constintsp=start+(end-start)*j/prm.sectors;" in cuh and "constintep=start+(end-start)*(j+1)/prm.sectors-1;" in cuh
    # the early-wrap pre-pass: the cloud's first 256 points, in both forms, through the one body
    assert cuh.count("constintpre_end=min(w1,256);") == 1 and cuh.count("constintpre_end=min(n,256);") == 1
    assert cuh.count("pre_end=") == 2 and cuh.count("prep_early_wraps(in,in_ring,pre_end,lane,") == 2
    assert cuh.count("atomicMin(&s_early[r],s_off[r]+seen+__popcll(below));") == 1
    # slices: multiples of 64, 16 per workgroup, one rule for both forms; four 64-point groups per iteration, one knob
    assert cuh.count("constintslice=") == 1 and cuh.count("constintslice=((n+S-1)/S+63)&~63;") == 1 and "S=16*G" in cuh
    assert cuh.count("prep_slice_bounds(n,16,wave,w0,w1);") == 1 and cuh.count("prep_slice_bounds(n,S,16*g+wave,w0,w1);") == 2
    assert cuh.count("#ifndefMSFL_PREP_GROUPS#defineMSFL_PREP_GROUPS4#endif") == 1 and cuh.count("#defineMSFL_PREP_GROUPS") == 1
    assert cuh.count("constexprintkPrepGroups=") == 1 and cuh.count("constexprintkPrepGroups=MSFL_PREP_GROUPS;") == 1
    assert "kGroups" not in cuh.replace("kPrepGroups", "")
    # the slice passes and the relative angle are written once: pass A's count, pass B's wrap test and time store
    assert cuh.count("atomicAdd(&cur[r],1);") == 1 and "atomicAdd(&s_cur" not in cuh
    assert cuh.count("atomicMin(&s_wrap[r],dst);") == 1
    assert cuh.count("out_pts[dst]=make_float4(p.x,p.y,p.z,(float)(aw/kPrepTwoPi*scan_period));") == 1 and cuh.count("out_pts[dst]=") == 1
    assert cuh.count("doublea=ori-start_ori+kPrepTwoPi;if(a>=kPrepTwoPi)a-=kPrepTwoPi;if(a>=kPrepTwoPi)a-=kPrepTwoPi;") == 1
    assert cuh.count("-atan2((double)p.y,(double)p.x)") == 1 and "rel_angle=[" not in cuh
    # the curvature tile and its halo
    assert "__shared__float4s_p[256+10];" in cuh and "constintg0=o+(int)blockIdx.x*256;" in cuh and "div_up(longest,256)" in host
    assert "if(i>=5&&i<N-5){" in cuh
    # the compact kernel's pieces
    assert "constexprintkCompactThreads=1024;" in cuh
    assert "for(intk0=g*4*kCompactThreads+tid;k0<total;k0+=G*4*kCompactThreads){" in cuh
    # G by batch size
    assert "intG=h->prep_split>0?h->prep_split:B<=16?16:B<=32?8:B<=64?4:B<=128?2:1;" in host
    assert "if(h->prep_split<=0&&G==1&&B>0&&(longlong)n_total/B>65536)G=2;" in host
    assert "if(g==1||g==2||g==4||g==8||g==16)h->prep_split=g;" in squeeze((csrc / "msfl_api.hip").read_text())
    G = lambda B: 16 if B <= 16 else 8 if B <= 32 else 4 if B <= 64 else 2 if B <= 128 else 1
    assert {B: G(B) for B in ec.B_EDGES} == ec.G_OF_B and sorted(set(ec.G_OF_B.values())) == sorted(ec.SPLITS)


def test_sector_sizes_at_the_pick_limits():
    S = ec.sector_sizes
    assert S(3083) == [512] * 6 and S(3084) == [512] * 5 + [513] and S(3088) == [512] + [513] * 5
    assert S(395) == [64] * 6 and S(17) == [1] * 6 and S(18) == [1] * 5 + [2] and S(16) == [] and S(11) == [] and S(10) == []
    assert min(S(3700)) > ec.PICK_SECTOR and min(S(8128)) > ec.PICK_SECTOR and max(S(800)) <= ec.PICK_SECTOR
    assert sum(S(8128)) == 8128 - 11
    for name in ALL:
        c = ec.case(name)
        if "sizes" in c.claim:
            assert c.claim["sizes"] == S(c.claim["lengths"][0]), name


@pytest.mark.parametrize("name", _group(("slices", "rings", "head", "badring")))
def test_prepare_cases(oracle, name):
    c = ec.case(name)
    pts, ring = c.clouds[0]
    f = oracle.extract_features(pts, ring)
    assert f["rc"] == c.status[0]
    if name.startswith("slices"):
        n = c.claim["n"]
        assert len(pts) == n == len(f["full"])
        for G, (filled, last) in c.claim["slices"].items():
            pop = [p for p in ec.slice_populations(n, G) if p]
            assert (len(pop), pop[-1]) == (filled, last), (name, G, len(pop), pop[-1])
        assert sum(ec.slice_populations(n, 1)) == sum(ec.slice_populations(n, 16)) == n
    if name == "slices_1023":                                   # 240 of 256 slices empty at G = 16, none of 16 at G = 1
        assert ec.slice_populations(1023, 16).count(0) == 240 and ec.slice_populations(1023, 1).count(0) == 0
    if name.startswith("rings"):
        assert tuple(np.unique(f["ring"])) == c.claim["ids"] == tuple(np.unique(ring))
    if name == "rings_one_bit":
        assert len(np.unique(ring[:64])) == 7 and all(bin(int(r)).count("1") == 1 for r in np.unique(ring))
    if name == "rings_all_128":
        assert np.all(np.bincount(f["ring"], minlength=128) == 20) and len(f["less_flat"]) + len(f["less_sharp"]) == 128 * 9      # all 128 rings are picked
    if name == "head_4001_invalid":
        valid = np.isfinite(pts[:, :3]).all(axis=1) & (np.linalg.norm(pts[:, :3].astype(np.float64), axis=1) >= 0.3)
        assert int(np.flatnonzero(valid)[0]) == c.claim["first_valid"] == 4001 and len(f["full"]) == c.claim["n_full"]
        for G in (2, 4, 8, 16):                                  # the first valid point lies in a later workgroup than the first
            assert 4001 // ec.slice_len(len(pts), G) // 16 >= 1, G
        assert np.sum(f["full"][:, 3] > ec.SCAN_PERIOD) > 0      # and the sweep wraps against ITS direction
    if name == "badring_last_point":
        assert ring[-1] == 128 and np.all(ring[:-1] < 128) and len(pts) == 5000
    if name == "badring_on_invalid_only":
        assert f["rc"] == 0 and len(f["full"]) == c.claim["n_full"] and sorted(ring[ring >= 128]) == [128, 300]


@pytest.mark.parametrize("name", _group(("wrap",)))
def test_planted_wraps_sit_at_their_claimed_index(oracle, name):
    """The oracle's first time above one scan period on every ring lies at the output index derived from the case's w alone; the
    predecessor of the wrap point is the one the case names, on the one-workgroup form and at G = 16."""
    c = ec.case(name)
    pts, ring = c.clouds[0]
    f = oracle.extract_features(pts, ring)
    off = _ring_offsets(f)
    assert f["rc"] == 0 and len(f["full"]) == len(pts)
    assert c.claim["wraps"] == ec.expected_wraps(ring, c.claim["w"])
    for r, k in c.claim["wraps"].items():
        t = f["full"][off[r]:off[r + 1], 3]
        above = np.flatnonzero(t > ec.SCAN_PERIOD)
        if k is None:
            assert len(above) == 0, (name, r)
            continue
        first = int(np.sum(ring[:k] == r))                     # the ring's points in front of k
        assert len(above) and above[0] == first and np.all(t[first:] > ec.SCAN_PERIOD), (name, r, above[:3], first)
    w = c.claim["w"]
    if w is not None:
        assert c.claim["wraps"][int(ring[w])] == w               # the chosen ring wraps exactly at w
        for G, path in c.claim["paths"].items():
            assert ec.wrap_path(ring, w, G) == path, (name, G, ec.wrap_path(ring, w, G))


def test_the_wrap_cases_cover_every_predecessor_path():
    """Paths 1-4 and 6 on the one-workgroup kernel (it has no earlier workgroup), 1, 2, 4, 5 and 6 at G = 16 (a slice of more than 256
    points needs a cloud of more than 65 536 there).  Early and late: the pre-pass ends behind cloud index 255."""
    seen = {1: set(), 16: set()}
    for name in _group(("wrap",)):
        c = ec.case(name)
        for G, path in c.claim["paths"].items():
            seen[G].add(path)
    assert seen[1] == {1, 2, 3, 4, 6} and seen[16] == {1, 2, 4, 5, 6}
    ws = {ec.case(n).claim["w"] for n in _group(("wrap",))}
    assert {2, 63, 64, 65, 255, 256, 257, 319, 320, 1023, 1024, ec.WRAP_N - 1, None} <= ws
    assert ec.slice_len(ec.WRAP_N, 1) == 320 and ec.slice_len(ec.WRAP_N, 16) == 64 and ec.slice_len(16385, 16) == 128
    both = ec.case("wrap_early_and_late").claim["wraps"]
    assert both == {2: 100, 9: 1000, 77: None}
    r = ec.case("wrap_grouped_1280").clouds[0][1]
    assert np.all(r[320:1280] == 9) and r[319] == r[1280] == 2    # three slices of 320 (fifteen of 64) without the ring in between


@pytest.mark.parametrize("name", _group(("ringlen", "ends")))
def test_ring_length_cases(oracle, name):
    c = ec.case(name)
    pts, ring = c.clouds[0]
    f = oracle.extract_features(pts, ring)
    off = _ring_offsets(f)
    assert f["rc"] == 0
    ids = c.claim.get("ring_ids", list(range(len(c.claim["lengths"]))))
    assert [int(off[r + 1] - off[r]) for r in ids] == c.claim["lengths"] and len(f["full"]) == sum(c.claim["lengths"])
    active = [n for n in c.claim["lengths"] if ec.sector_bounds(n)]
    if name in ("ringlen_10", "ringlen_11", "ringlen_16"):
        assert not active and len(f["less_flat"]) == 0 and len(f["sharp"]) == 0
    if name == "ringlen_17":
        assert len(f["less_flat"]) + len(f["less_sharp"]) >= 6 and len(f["sharp"]) >= 1
    if name == "ringlen_1_to_24":
        assert [n for n in c.claim["lengths"] if ec.sector_bounds(n)] == list(range(17, 25))
    for q in c.claim.get("corners", []):                         # a corner at the ring's first / last pickable position, eleven points suppressed
        for r in ids:
            s = int(off[r])
            assert s + q in f["sharp"], (name, r, q)
            assert np.all(f["label"][s + q - 5:s + q] == 2) and np.all(f["label"][s + q + 1:s + q + 6] == 2) and f["label"][s + q] == 1
    if "corners" in c.claim:
        n = c.claim["lengths"][0]
        assert c.claim["corners"] == [5, n - 7] and n - 7 + 5 == n - 2        # the windows are [0, 10] and [n - 12, n - 2]


def _pickable(f, off, ids):
    m = np.zeros(len(f["label"]), bool)
    for r in ids:
        if off[r + 1] - off[r] >= 17:
            m[off[r] + 5:off[r + 1] - 6] = True
    return m


def _sector_start(n, pos):
    return ec.sector_bounds(n)[ec.sector_of(n, pos)][0]


@pytest.mark.parametrize("name", _group(("tie", "flat")))
def test_tie_cases_tie_where_they_claim(oracle, name):
    """Each claimed pair has equal curvature bits, stands in the oracle's list in the claimed order (corner pass: the higher index
    first; flat pass: the lower), and its two positions share a lane (sp + lane + 64 t) or do not, as claimed."""
    c = ec.case(name)
    pts, ring = c.clouds[0]
    n = c.claim["lengths"][0]
    f = oracle.extract_features(pts, ring)
    assert f["rc"] == 0 and len(f["full"]) == n
    bits = f["curvature"].view(np.uint32)
    for key, lst, higher_first in (("sharp_pairs", f["sharp"], True), ("flat_pairs", f["flat"], False)):
        pairs = c.claim.get(key, [])
        lst = lst.tolist()
        for a, b, lanes in pairs:
            assert bits[a] == bits[b] and (a > b) == higher_first, (name, a, b)
            assert lst.index(b) == lst.index(a) + 1, (name, key, a, b)
            sp = _sector_start(n, a)
            assert sp == _sector_start(n, b)
            assert ((a - sp) % 64 == (b - sp) % 64) == (lanes == "same"), (name, a, b, sp)
    pairs = c.claim.get("sharp_pairs", []) + c.claim.get("flat_pairs", [])
    lanes = {p[2] for p in pairs}
    if name.startswith("tie_") and name.split("_")[2] in ("7", "16") and n >= 800:
        assert lanes == {"cross"} and len(pairs) == 6
    if name.startswith("tie_3083_64") or name.startswith("tie_3700_64"):
        assert lanes == {"same"} and len(pairs) == 6
    if name.startswith("tie_3083_64"):
        assert pairs[:2] == [(512, 448, "same"), (1024, 960, "same")]
    if name == "tie_800_16_s8":
        assert pairs[0] == (128, 112, "cross")
    if name.startswith("tie_") and c.claim["step"] == 0.25 and n >= 800:
        assert len(f["less_sharp"]) == 120                        # the 20-per-sector cap, in every sector
    if name.startswith("flat_inlane"):
        assert lanes == {"same"} and len(pairs) == 18 and np.all(bits[ec.inlane_flat_positions(n)] == 0)
        cand = np.flatnonzero((f["curvature"] < 0.1) & _pickable(f, _ring_offsets(f), [0]))
        assert cand.tolist() == ec.inlane_flat_positions(n)       # nothing else is a flat candidate
    if name.startswith("flat_cross"):
        assert lanes == {"cross"} and len(pairs) == 18


@pytest.mark.parametrize("name", _group(("seam",)))
def test_seam_cases(oracle, name):
    c = ec.case(name)
    pts, ring = c.clouds[0]
    n = c.claim["lengths"][0]
    f = oracle.extract_features(pts, ring)
    sec = ec.sector_bounds(n)
    assert f["rc"] == 0
    for q in c.claim["corners"]:
        assert q in f["sharp"] and f["label"][q] == 1
        assert np.all(f["label"][q - 5:q] == 2) and np.all(f["label"][q + 1:q + 6] == 2)      # back = fwd = 5
    if "window_bits" in c.claim:
        assert c.claim["window_bits"] == [27, 28, 29, 30, 31]
        return
    q = c.claim["corners"][0]
    j = ec.sector_of(n, q)
    assert np.all(f["label"][c.claim["label2"]] == 2)
    if "no_flat_in" in c.claim:                                  # the corner is sector j's last point; the five behind it were sector j + 1's only flat candidates
        assert q == sec[j][1] and c.claim["no_flat_in"] == sec[j + 1]
        sp, ep = sec[j + 1]
        cand = np.flatnonzero(f["curvature"][sp:ep + 1] < 0.1) + sp
        assert cand.tolist() == list(range(q + 1, q + 6))
        assert not np.any((f["flat"] >= sp) & (f["flat"] <= ep)) and np.sum((f["flat"] >= sec[j][0]) & (f["flat"] <= q)) == 4
    else:                                                        # the corner is sector j's first point; sector j - 1's less-flat list keeps what it relabels
        assert q == sec[j][0] and j >= 1
        assert set(c.claim["less_flat_has"]) <= set(f["less_flat"].tolist())
        assert np.all(f["label"][c.claim["less_flat_has"]] == 2)
    if n == 3084:
        assert ec.sector_sizes(n)[4] == ec.PICK_SECTOR and ec.sector_sizes(n)[5] == ec.PICK_SECTOR + 1 and j in (4, 5)
    if n == 3085:                                                # a re-read sector in front of an LDS one
        assert ec.sector_sizes(n) == [512, 512, 513, 512, 512, 513] and j in (2, 3)


def test_tile_batch_has_the_claimed_n_full(oracle):
    c = ec.case("tiles_26_scans")
    assert set(c.claim["n_full"]) == set(range(250, 263)) | set(range(506, 519))
    for (pts, ring), nf, raw in zip(c.clouds, c.claim["n_full"], c.claim["raw"]):
        f = oracle.extract_features(pts, ring)
        assert f["rc"] == 0 and len(f["full"]) == nf and len(pts) == raw == nf + 300
        assert -(-raw // 256) > -(-nf // 256) or raw - nf > 256      # surplus tiles: the raw size exceeds n_full by more than a tile


@pytest.mark.parametrize("name", list(ec.COMPACT))
def test_compact_cases_have_the_claimed_less_flat_total(oracle, name):
    c = ec.case(name)
    pts, ring = c.clouds[0]
    f = oracle.extract_features(pts, ring)
    assert f["rc"] == 0 and len(f["sharp"]) == 0 and len(f["less_sharp"]) == 0
    assert len(f["less_flat"]) == c.claim["less_flat"] == sum(n - 11 for n in c.claim["lengths"])
    assert c.claim["less_flat"] in (4 * 1024 - 1, 4 * 1024, 4 * 1024 + 1, 16 * 4 * 1024 - 1, 16 * 4 * 1024, 16 * 4 * 1024 + 1)
    assert len(pts) <= 16 * 4108


def test_batch_cases(oracle):
    c = ec.case(ec.REFUSED_BATCH)
    got = [oracle.extract_features(p, r)["rc"] for p, r in c.clouds]
    assert got == c.claim["oracle_status"]
    # the kernel's statuses are the oracle's, but for the ring beyond the on-chip capacity, which the oracle extracts
    assert [s for s, o in zip(c.status, got) if s != o] == [ec.CAPACITY] and len(c.clouds[4][0]) == ec.RING_CAPACITY + 1
    assert len(c.clouds[1][0]) == 0
    for B in ec.B_EDGES:
        sizes = [len(p) for p, _ in ec.batch_of(B)]
        assert len(sizes) == B and min(sizes) >= 40 and max(sizes) <= 300
    assert all(oracle.extract_features(p, r)["rc"] == 0 for p, r in ec.tiny_pool())
