"""CPU: every case of tests/voxel_limit_cases.py sits where its name claims.

The voxel filter hands a cloud from form to form by flags written on the device; a case that drifts off its edge (one run fewer, a
bounding box one cell narrower) would still pass its GPU test, on another path.  For every case the model of
tests/voxel_form_model.py must therefore reproduce the case's hand-overs, reasons included, its figures exactly, and no branch the
case does not claim; the oracle must find the voxel count the construction implies.  The GPU counterpart is
tests/test_gpu_voxel_limits.py.
"""
import itertools
import pathlib
import re

import numpy as np
import pytest

from tests import voxel_form_model as vm
from tests import voxel_limit_cases as vc

HANDLES = ("default", "no_big", "global")


def _one_point_analysis():
    return dict(n=1, finite_xyz=True, finite_w=True, coord_abs_max=0.0, cells=1, runs_g=1, runs=1)


def _sum_in_order(p):
    s = np.zeros(4, np.float32)
    for q in p: s = s + q
    return s


def test_the_table_is_deterministic():
    for name in ("P_65", "K_257x256x1_S", "W_S_513"):
        a = vc.case(name).pts.copy()
        vc.case.cache_clear()
        assert np.array_equal(a.view(np.uint32), vc.case(name).pts.view(np.uint32))
    assert len(set(vc.NAMES)) == len(vc.NAMES)


def test_the_edges_are_the_kernels_constants():
    """The figures in the case names are the model's constants: n, n + 1 around each."""
    F = vm.FORMS
    assert (F["S"]["max_points"], F["L"]["max_points"], F["B"]["max_points"]) == (4096, 65535, 131071)
    assert (F["S"]["max_runs"], F["L"]["max_runs"], F["B"]["max_runs"]) == (2048, 12288, 65536)
    assert (F["S"]["multi_cap"], F["L"]["multi_cap"], F["B"]["multi_cap"]) == (960, 3840, 3840)
    assert (vm.coord_limit("S"), vm.coord_limit("L"), vm.coord_limit("B")) == (8190, 8190, 4094)
    assert (vm.max_chunks("S"), vm.max_chunks("L"), vm.max_chunks("B")) == (256, 1024, 2048)
    for form in "SLB":        # kBigCap overflow is unreachable: that many big voxels hold more points than the form's largest cloud
        assert F[form]["big_cap"] * (vm.BIG_VOXEL + 1) > F[form]["max_points"]
        assert F[form]["max_points"] <= vm.max_chunks(form) * vm.CHUNK            # the chunk table covers the largest cloud
        assert F[form]["max_points"] < (1 << F[form]["first_bits"])                # a run's first point fits its field


def test_the_models_constants_are_the_kernels():
    """The model's constants and comparisons, read out of the kernel source: the GPU test cannot see which form served a cloud
    (every form computes the same bits), so a limit moved in msfl_extract.cuh alone would leave every case passing on another path.
    This reads the constants and the sense (< against <=) of each limit's test from the source text; it does not compile
    anything, so it pins what is written there, not what it does."""
    csrc = pathlib.Path(__file__).resolve().parent.parent / "msf_loam_amd" / "csrc"
    squeeze = lambda t: re.sub(r"\s+", "", t)
    cuh, host = squeeze((csrc / "msfl_extract.cuh").read_text()), squeeze((csrc / "msfl_api_stage_ab.inc").read_text())
    F = vm.FORMS
    num = lambda pattern: int(re.search(pattern, cuh).group(1))
    # the three instantiations: <waves, runs per wavefront>
    for form, inst, text in (("S", "voxel_cloud_lds_kernel<%d,%d>", host), ("L", "voxel_cloud_lds_kernel<%d,%d>", host),
                             ("B", "voxel_cloud_body<%d,%d,true,true>", cuh)):
        assert inst % (F[form]["waves"], F[form]["max_runs"] // F[form]["waves"]) in text, form
    assert "kVoxMaxRuns=kVoxWaves*kVoxRunsPerWave;" in cuh
    assert num(r"constexprintkVoxSmallPoints=(\d+);") == F["S"]["max_points"]
    assert num(r"constexprintkVoxMaxPoints=(\d+);") == F["L"]["max_points"]
    assert "kMaxPoints=kBig?%d:(kVoxWaves<16?kVoxSmallPoints:kVoxMaxPoints);" % F["B"]["max_points"] in cuh
    assert "kCB=kBig?%d:%d,kFB=kBig?%d:%d," % (F["B"]["coord_bits"], F["L"]["coord_bits"], F["B"]["first_bits"], F["L"]["first_bits"]) in cuh
    assert (F["S"]["coord_bits"], F["S"]["first_bits"]) == (F["L"]["coord_bits"], F["L"]["first_bits"])
    assert "kCoordOff=1<<(kCB-1);" in cuh
    assert "kMaxChunks=kVoxWaves*(kBig?128:64);" in cuh
    assert num(r"#defineMSFL_VOX_BIG_VOXEL(\d+)/") == vm.BIG_VOXEL
    for form in "SLB":
        assert "kMultiCap=kVoxWaves*%d,kBigCap=kVoxWaves*%d;" % (F[form]["multi_cap"] // F[form]["waves"], F[form]["big_cap"] // F[form]["waves"]) in cuh
    # the sense of each limit's test, as verdict() and analyse() restate it
    assert "if(n>kMaxPoints){if(tid==0){flags[b]=kSmall?5:4;" in cuh                                          # verdict: n > max_points
    assert "if(s_alloc>kVoxMaxRuns)flag=max(flag,kSmall?5:4);" in cuh                                         # runs > max_runs
    assert cuh.count("fabsf(f%d)<(float)(kCoordOff-1)" % 0) == 1 and all("fabsf(f%d)<(float)(kCoordOff-1)" % k in cuh for k in (1, 2))
    assert "if(later>kBigVoxel){" in cuh and "if(at<kBigCap){" in cuh and "if(at<kMultiCap){" in cuh
    assert "constexprintkBigVoxel=MSFL_VOX_BIG_VOXEL" in cuh
    assert "intseg=((n+kVoxWaves-1)/kVoxWaves+63)&~63;" in cuh
    assert "while((1ll<<nbits)<cells)nbits++;" in cuh and "for(intshift=0;shift<nbits;shift+=%d){" % vm.RADIX_BITS in cuh
    assert cuh.count("if(cells>0x7fffffffLL)") >= 2                                                           # the one-workgroup forms' and the device-wide form's
    assert "if(!(fabsf(flo)<1e9f&&fabsf(fhi)<1e9f)){" in cuh and vm.G_COORD_LIMIT == 1e9


@pytest.mark.parametrize("name", [n for n in vc.NAMES if n[0] != "Q"])
def test_case_sits_on_its_claimed_side(oracle, name):
    c = vc.case(name)
    clouds = c.clouds
    routes = {h: vm.route_batch(clouds, c.leaf, h) for h in HANDLES}
    a = routes["default"]["analyses"][c.target]
    # the hand-overs on the default handle, with the reason for each
    assert routes["default"]["path"][c.target] == [(f, fl) for f, fl, _ in c.path], routes["default"]["path"][c.target]
    for form, flag, why in c.path:
        v = vm.g_verdict(a) if form == "G" else vm.verdict(a, form)
        assert (v["flag"], v["why"]) == (flag, why), (form, v["flag"], v["why"])
    for h in HANDLES:
        assert routes[h]["status"] == c.status, h
        assert routes[h]["served"][c.target] == vc.serve_on(c.form, h), (h, routes[h]["served"][c.target])
        for b in range(len(clouds)):                                   # the clouds around a refused one are ordinary
            if b != c.target:
                assert routes[h]["served"][b] in ("S", "G")
    # the figures that put the case on its edge, and no branch it does not claim
    served = vm.verdict(a, c.form) if c.form in vm.FORMS else {}
    for key, want in c.claim.items():
        got = a[key] if key in a else served[key]
        assert got == want, (key, got, want)
    if c.form in vm.FORMS:
        for key in ("multi_overflow", "big_overflow", "n_big"):
            assert served[key] == c.claim.get(key, 0), (key, served[key])
        assert served["pool_left"] >= 0
    if c.voxels is not None:
        assert a["voxels"] == c.voxels
        assert len(oracle.voxel_grid(clouds[c.target], c.leaf)) == c.voxels
    if c.status == "OK":
        print("%-22s %s n=%d runs=%d voxels=%d multi=%d later_max=%d cells=%d (%d bits, %d passes)" % (
            name, "".join(f for f, _, _ in c.path), a["n"], a["runs"], a["voxels"], a["multi"], a["later_max"], a["cells"], a["nbits"], a["radix_passes"]))


@pytest.mark.parametrize("name", [n for n in vc.NAMES if n[0] == "K"])
def test_k_cases_need_the_sorts_last_pass(name):
    """Two voxels whose indices differ only in the top radix digit arrive in descending order: a sort that drops its last pass
    leaves them in arrival order, which is the wrong one.  Also the 8 / 9, 16 / 17, 24 / 25 bit edges themselves."""
    c = vc.case(name)
    a = vm.analyse(c.clouds[0], c.leaf)
    shift = vm.RADIX_BITS * (a["radix_passes"] - 1)
    assert (1 << a["nbits"]) >= a["cells"] > (1 << (a["nbits"] - 1))
    cell = a["cell"][-400:]
    low = cell & ((1 << shift) - 1)
    hit = 0
    for i in range(len(cell)):
        later = np.flatnonzero((low[i + 1:] == low[i]) & (cell[i + 1:] < cell[i]))
        hit += len(later)
    assert hit >= 1, "no pair that only the last pass orders"
    assert int(a["cell"].max()) == a["cells"] - 1 and int(a["cell"].min()) == 0          # both corners are there: the box is the claimed one


@pytest.mark.parametrize("name", [n for n in vc.NAMES if n[0] == "W"])
def test_w_cases_deliver_the_later_points_across_every_seam(name):
    """The big voxel's later points come as runs of 1, 2, 63 and 64, as runs a chunk boundary cut, and across a wavefront-slice
    boundary of the serving form; and its centroid depends on the order of summation in every lane (forward f32, reversed f32 and
    f64 all differ), so a walk that adds the right points in another order cannot pass."""
    c = vc.case(name)
    form, later, n_vox, _, _, _ = vc.W_SPEC[name]
    cloud = c.clouds[0]
    a = vm.analyse(cloud, c.leaf)
    _, vcells = vc.w_cells(later, n_vox, a["n"], vc.W_SPEC[name][4])
    f = vm.voxel_coords(cloud, c.leaf).astype(np.int64)
    seg, _ = vm.slices(a["n"], form)
    across_slice = checked = 0
    for v in vcells:
        mine = np.all(f == v, axis=1)
        k = np.flatnonzero(mine)
        assert len(k) == later + 1
        assert k[1] == k[0] + 2                                            # a one-point first run, then some other voxel's point
        runs = [(s, l) for s, l in zip(a["run_start"], a["run_len"]) if mine[s]]
        lens = [l for _, l in runs]
        assert lens[0] == 1 and sum(lens[1:]) == later
        assert {1, 2, 63, 64} <= set(lens[1:])
        assert any(s % 64 == 0 and mine[s - 1] for s, _ in runs[1:])      # a run that only the chunk boundary opened
        across_slice += sum(1 for s, _ in runs[1:] if s % seg == 0 and mine[s - 1])
        p = cloud[k]
        fwd, rev = np.zeros(4, np.float32), np.zeros(4, np.float32)
        for q in p: fwd = fwd + q
        for q in p[::-1]: rev = rev + q
        exact = p.astype(np.float64).sum(axis=0).astype(np.float32)
        cnt = np.float32(len(p))
        for other in (rev, exact):                                        # all four lanes, every such voxel; sums and centroids
            assert np.all(fwd.view(np.uint32) != other.view(np.uint32)), (v, fwd, other)
            assert np.all((fwd / cnt).view(np.uint32) != (other / cnt).view(np.uint32)), (v, fwd / cnt, other / cnt)
        checked += 1
    assert checked == n_vox
    assert across_slice >= 1, "no run of a big voxel continues across a wavefront-slice boundary"


def test_z_cases_come_out_as_positive_zero(oracle):
    """0.f + x: a lone -0 leaves the filter as +0, and x + (-x) is +0; the oracle (pcl's CentroidPoint arithmetic) says so too."""
    lone = oracle.voxel_grid(vc.case("Z_lone_negative_zero").pts, 0.5)
    assert lone.shape == (1, 4) and not lone.view(np.uint32).any()
    assert np.all(vc.case("Z_lone_negative_zero").pts.view(np.uint32) == 0x80000000)
    two = oracle.voxel_grid(vc.case("Z_two_runs_cancel").pts, 0.5)
    assert two.shape == (2, 4) and not two[0].view(np.uint32).any()


@pytest.mark.parametrize("name", list(vc.Q_SPEC))
def test_q_cases_fill_the_key(oracle, name):
    """65 536 / 65 537 clouds, one of them spanning 1100^3 cells: 31 + 17 + 16 = 64 key bits (the run number still rides in the
    key) and 31 + 17 + 17 = 65 (the (key, value) sort)."""
    c = vc.case(name)
    sizes = np.diff(c.off)
    n_clouds, revisit = vc.Q_SPEC[name]
    more = {c.target: 2, vc.Q_REVISIT_CLOUD: 66} if revisit else {c.target: 2}
    assert len(sizes) == n_clouds and all(sizes[b] == (more.get(b, 1)) for b in range(n_clouds))
    rest = np.delete(c.pts, [c.off[c.target], c.off[c.target] + 1], axis=0)
    assert np.abs(vm.voxel_coords(rest, c.leaf)).max() <= 10 and np.isfinite(rest).all()
    two = vm.analyse(c.clouds[c.target], c.leaf)
    assert vm.verdict(two, "S")["flag"] == 0 and vm.g_verdict(two)["flag"] == 0
    an = [_one_point_analysis() for _ in sizes]
    an[c.target] = two
    if revisit:
        # a voxel that the (key, value) sort has to keep in arrival order: three runs, and summed in any other order of its runs
        # the centroid differs in all four lanes
        cloud = c.clouds[vc.Q_REVISIT_CLOUD]
        an[vc.Q_REVISIT_CLOUD] = r = vm.analyse(cloud, c.leaf)
        assert (r["runs_g"], r["voxels"], r["multi"], r["later_max"]) == (5, 3, 1, 40)
        runs = [list(k) for k in vc.Q_REVISIT_RUNS]
        f = vm.voxel_coords(cloud, c.leaf)
        assert sorted(sum(runs, [])) == np.flatnonzero(np.all(f == f[0], axis=1)).tolist()
        fwd = _sum_in_order(cloud[sum(runs, [])])
        orders = [o for o in itertools.permutations(runs) if list(o) != runs]
        assert len(orders) == 5
        for o in orders:
            other = _sum_in_order(cloud[sum(o, [])])
            assert np.all(fwd.view(np.uint32) != other.view(np.uint32)), (o, fwd, other)
            assert np.all((fwd / np.float32(64)).view(np.uint32) != (other / np.float32(64)).view(np.uint32)), o
    key = vm.g_key(an)
    for k, want in c.claim.items():
        assert key[k] == want, (k, key[k], want)
    assert len(oracle.voxel_grid(c.clouds[c.target], c.leaf)) == c.voxels
