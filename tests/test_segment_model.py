"""CPU: the numpy model of the scan segmentation (tests/segment_numpy.py) against hand-written expectations, against itself (the two
statements of the components) and against the library's host-only table call; and what the rule is worth on the synthetic sweeps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_cases as sc
import segment_numpy as sn


def _capi():
    from msf_loam_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def _c_config(capi, cfg):
    return capi.SegmentConfig(**vars(cfg))


HAND = sc.hand_scenes()
STRESS = sc.stress_scenes()


@pytest.mark.parametrize("scene", HAND, ids=[s[0] for s in HAND])
def test_hand_scene_classes(scene):
    name, pts, ring, cfg, want = scene
    for method in ("union", "flood"):
        out = sn.segment_scan(pts, ring, cfg, method=method)
        assert out["cls"].tolist() == want.tolist(), (name, method)
        assert out["info"][:5].tolist() == np.bincount(want, minlength=5).tolist()
        kept = np.isin(want, (sn.GROUND, sn.SEGMENT))
        assert np.array_equal(np.isnan(out["masked"][:, 0]), ~kept) and sn.same_bits(out["masked"][kept], pts[kept])
        assert sn.same_bits(out["masked"][:, 3], pts[:, 3]) and out["info"][8] == kept.sum()


def test_hand_scene_components():
    by = {s[0]: s for s in HAND}
    _, pts, ring, cfg, _ = by["box"]
    out = sn.segment_scan(pts, ring, cfg)
    assert set(out["segment"].tolist()) == {4 * 64 + 10} and out["info"][5:8].tolist() == [40, 1, 1]
    _, pts, ring, cfg, _ = by["two_boxes"]
    out = sn.segment_scan(pts, ring, cfg)
    assert set(out["segment"].tolist()) == {4 * 64 + 10, 4 * 64 + 16} and out["info"][6:8].tolist() == [2, 2]
    _, pts, ring, cfg, _ = by["wrap"]
    out = sn.segment_scan(pts, ring, cfg)
    assert set(out["segment"].tolist()) == {4 * 64} and out["info"][6:8].tolist() == [1, 1]
    _, pts, ring, cfg, _ = by["shadowed"]
    out = sn.segment_scan(pts, ring, cfg)
    assert out["segment"].tolist() == [-1, 5 * 64 + 40, 6 * 64 + 41, -1]
    _, pts, ring, cfg, _ = by["level_ground"]
    out = sn.segment_scan(pts, ring, cfg)
    assert out["info"].tolist() == [0, 0, 256, 0, 0, 256, 0, 0, 256, 0] and set(out["segment"].tolist()) == {-1}


@pytest.mark.parametrize("scene", STRESS, ids=[s[0] for s in STRESS])
def test_component_shapes_both_ways(scene):
    name, pts, ring, cfg, want, n_comp = scene
    a = sn.segment_scan(pts, ring, cfg, method="union")
    b = sn.segment_scan(pts, ring, cfg, method="flood")
    for k in a:
        assert sn.same_bits(a[k], b[k]), (name, k)
    assert a["info"][6] == n_comp and a["info"][7] == n_comp and a["cls"].tolist() == want.tolist()
    assert len(set(a["segment"].tolist())) == n_comp


@pytest.mark.parametrize("shape", [(2, 4), (6, 32), (16, 64), (16, 1800)])
def test_random_images_both_ways(shape):
    for seed in (1, 2):
        pts, ring, cfg = sc.random_image(seed, *shape)
        a = sn.segment_scan(pts, ring, cfg, method="union")
        b = sn.segment_scan(pts, ring, cfg, method="flood")
        for k in a:
            assert sn.same_bits(a[k], b[k]), (shape, seed, k)
        assert a["info"][:5].sum() == len(pts)
        if shape[0] >= 16:
            assert all(a["info"][k] > 0 for k in range(5)), a["info"]      # the generator reaches every class


def test_all_hand_and_ragged_cases_agree_both_ways():
    pts, ring, off, cfg = sc.ragged_batch()
    a = sn.segment_scans(pts, ring, off, cfg, method="union")
    b = sn.segment_scans(pts, ring, off, cfg, method="flood")
    for k in a:
        assert sn.same_bits(a[k], b[k]), k
    assert a["info"][5, :5].sum() == 0 and a["info"][17, :5].sum() == 1
    assert np.array_equal(a["info"][:, :5].sum(axis=1), np.diff(off))


def test_tables_equal_the_librarys():
    capi = _capi()
    cfgs = [sn.config(), sc.hand_config(), sc.stress_config(), sn.config(n_col=2048, n_row=128, ground_rows=50, ground_angle_deg=7.5, segment_angle_deg=45.0),
            sn.config(n_col=4, n_row=2, ground_rows=1), sn.config(n_row=5, row_elev_deg=[-25.0, -11.5, -3.0, 1.0, 15.25], ground_rows=2)]
    for cfg in cfgs:
        mine = sn.tables(cfg)
        theirs = capi.segment_tables(_c_config(capi, cfg))
        for a, b in zip(mine, theirs):
            assert sn.same_bits(a, b), vars(cfg)


def test_default_config_is_the_models():
    capi = _capi()
    c = capi.SegmentConfig()
    for k, v in sn.DEFAULTS.items():
        got = getattr(c, k)
        assert (list(got) == list(v)) if k == "up" else (got == (v if v is None or isinstance(v, int) else np.float32(v))), k


BAD = [dict(n_col=2), dict(n_col=2050), dict(n_col=63), dict(n_row=1), dict(n_row=129), dict(elev_low_deg=-90.0), dict(elev_high_deg=90.0),
       dict(elev_low_deg=15.0), dict(elev_low_deg=float("nan")), dict(min_range=-1.0), dict(min_range=100.0), dict(max_range=float("inf")),
       dict(ground_rows=-1), dict(ground_rows=16), dict(ground_angle_deg=0.0), dict(ground_angle_deg=90.0), dict(segment_angle_deg=0.0),
       dict(segment_angle_deg=90.0), dict(segment_angle_deg=float("nan")), dict(up=(0.0, 0.0, 0.0)), dict(up=(0.0, 0.0, 2.0)),
       dict(up=(float("nan"), 0.0, 1.0)), dict(min_points=0), dict(min_points_tall=0), dict(min_rows_tall=0), dict(keep_classes=-1),
       dict(keep_classes=32), dict(row_elev_deg=[0.0] * 16), dict(row_elev_deg=list(range(-8, 7)) + [95.0]),
       dict(row_elev_deg=[float("nan")] + list(range(1, 16)))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(b) + "=" + str(list(b.values())[0])[:12] for b in BAD])
def test_tables_refuse_a_configuration_outside_its_limits(bad):
    capi = _capi()
    with pytest.raises(capi.MsflError) as e:
        capi.segment_tables(capi.SegmentConfig(**bad))
    assert e.value.status == capi.BAD_ARG


def test_columns_are_centred_on_the_beams():
    """A beam of the synthetic sensor lies in the middle of its column: range noise moves no return into a neighbour's pixel."""
    pts, ring = sc.sweep("room")
    cfg = sn.config()
    out = sn.segment_scan(pts, ring, cfg)
    assert out["info"][sn.SHADOWED] == 0 and out["info"][sn.NONE] == 0 and out["info"][5] == len(pts)


@pytest.mark.parametrize("kind", ["room", "outdoor"])
def test_model_worth_on_the_synthetic_sweeps(kind):
    """Floors well under the f64 prototype's figures: ground returns labelled GROUND, volumetric returns OUTLIER, wall returns kept."""
    cfg = sn.config()
    for k in range(3):
        pts, ring, hit = sc.sweep(kind, k, with_kind=True)
        out = sn.segment_scan(pts, ring, cfg)
        if k == 0:
            flood = sn.segment_scan(pts, ring, cfg, method="flood")
            assert all(sn.same_bits(out[name], flood[name]) for name in out)
        cls = out["cls"]
        frac = lambda kind_id, c: float(np.mean(cls[hit == kind_id] == c))
        print(kind, k, "ground->GROUND %.3f" % frac(0, sn.GROUND), "wall->SEGMENT %.3f" % frac(1, sn.SEGMENT),
              "volume->OUTLIER %.3f" % (frac(3, sn.OUTLIER) if (hit == 3).any() else -1.0), "shadowed %.4f" % np.mean(cls == sn.SHADOWED))
        assert frac(0, sn.GROUND) >= 0.90
        assert frac(1, sn.SEGMENT) >= 0.60
        assert np.mean(cls == sn.SHADOWED) <= 0.01
        if kind == "outdoor":
            assert (hit == 3).sum() > 1000 and frac(3, sn.OUTLIER) >= 0.70
