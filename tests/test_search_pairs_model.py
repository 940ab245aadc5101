"""CPU: what msfl_search_pairs rests on, without a GPU.  The pairs of one call share their config, so their geometries differ in
`origin` only (the kernels take one geometry and a table of origins); the symbol and its prototype; the refusals that the
geometry rule and the argument check make before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import search_numpy as sn
from tests import search_pairs_cases as spc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(spc.CASES, five=spc.FIVE)


def _config(cfg, **kw):
    from msf_loam_amd import capi
    c = capi.SearchConfig(step=cfg.step, half=cfg.half, n_yaw=cfg.n_yaw, yaw_min=cfg.yaw_min, yaw_step=cfg.yaw_step, yaw_wraps=cfg.yaw_wraps,
                          dilate=cfg.dilate, range=cfg.range, nms_cells=cfg.nms_cells, nms_yaws=cfg.nms_yaws, max_volume_bytes=cfg.max_volume_bytes)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _fields(g):
    return {name: (list(getattr(g, name)) if hasattr(getattr(g, name), "__len__") else getattr(g, name)) for name, _ in g._fields_}


@pytest.mark.parametrize("name", sorted(ALL))
def test_geometries_of_a_call_differ_in_origin_only(name):
    from msf_loam_amd import capi
    case = ALL[name]()
    geoms = []
    for p in range(case.P):
        s, g = capi.search_geometry(case.guess[p], _config(case.cfg), len(case.c[p]), len(case.s[p]))
        assert s == capi.OK
        want = sn.geometry(case.guess[p], case.cfg, len(case.c[p]), len(case.s[p]))
        assert np.array_equal(np.array(list(g.origin), np.float32), want.origin) and g.n_hypotheses == want.H
        geoms.append(_fields(g))
    for g in geoms[1:]:
        for k in g:
            if k not in ("origin", "scratch_bytes"):       # (scratch_bytes counts the pair's own features)
                assert g[k] == geoms[0][k], k
    if name == "far_and_negative":
        o = np.array([g["origin"] for g in geoms])
        assert np.abs(o[0] - o[1]).max() > 2000.0 and (o[1] < 0).all()


def test_symbol_and_prototype():
    from msf_loam_amd import capi
    lib = capi.load()
    fn = lib.msfl_search_pairs
    assert "msfl_search_pairs" in capi.EXPORTED and capi.PROTOTYPES["msfl_search_pairs"] == "i:pipppppppippi"
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    header = open(os.path.join(ROOT, "include", "msfl_c_api.h")).read()
    decl = re.search(r"msfl_status\s+msfl_search_pairs\s*\(([^;]*)\)\s*;", header).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == 13
    kinds = "".join("p" if "*" in p else "i" for p in params)
    assert kinds == capi.PROTOTYPES["msfl_search_pairs"].split(":")[1]
    # declared after msfl_relocalize, as the section order of the header has it
    assert header.index("msfl_status msfl_relocalize(") < header.index("msfl_status msfl_search_pairs(")
    names = list(capi.PROTOTYPES)
    assert names.index("msfl_search_pairs") == names.index("msfl_relocalize") + 1


def test_refusals_that_need_no_device():
    from msf_loam_amd import capi
    lib = capi.load()
    case = spc.CASES["far_and_negative"]()
    cfg = _config(case.cfg)
    # the geometry rule, pair by pair: what the call answers is what msfl_search_geometry answers for the first pair it refuses
    bad = case.guess.copy(); bad[2, 1] = np.nan
    status = [capi.search_geometry(bad[p], cfg, len(case.c[p]), len(case.s[p]), allow=(capi.BAD_ARG,))[0] for p in range(case.P)]
    assert status == [capi.OK, capi.OK, capi.BAD_ARG]
    tiny = _config(case.cfg, max_volume_bytes=64)
    assert [capi.search_geometry(case.guess[p], tiny, 1, 1, allow=(capi.CAPACITY,))[0] for p in range(case.P)] == [capi.CAPACITY] * case.P
    zero = _config(case.cfg, step=0.0)
    assert capi.search_geometry(case.guess[0], zero, 1, 1, allow=(capi.BAD_ARG,))[0] == capi.BAD_ARG
    # no handle: refused before anything else is looked at
    off = np.zeros(2, np.int32)
    cand = np.zeros(1, capi.POSE_CANDIDATE_DTYPE)
    n_out = np.zeros(1, np.int32)
    assert lib.msfl_search_pairs(None, 1, None, off.ctypes.data, None, off.ctypes.data, case.guess.ctypes.data, ctypes.addressof(cfg),
                                 cand.ctypes.data, 1, n_out.ctypes.data, None, capi.MEM_HOST) == capi.BAD_ARG
    # the binding's own checks
    with pytest.raises(ctypes.ArgumentError):
        lib.msfl_search_pairs(None, 1.5, None, None, None, None, None, None, None, 1, None, None, 0)
