#!/usr/bin/env python3
"""Map-store cost against map size: msfl_grid_insert_scan / msfl_grid_get_surrounded timed while the map grows.

Each inserted "scan" is 6 000 points on a patch of ground and walls that moves 2 m per scan (a vehicle's down-sampled
less-flat list lands in ~150 cells of 3 m); the map therefore grows by a few thousand voxels per scan.  Prints one JSON
line per checkpoint: map points / cells, ms per insert and ms per surround query (wall clock around the C call, host
buffers, so the figures include the PCIe copy of the scan and, for the query, of the result).

--window HX,HY,HZ: the windowed-map leg instead.  A translating stream of 16-beam-sized scans (the same scan_at clouds) is
inserted twice, into a store that is cropped to the window after every insert (msfl_grid_crop around the scan's centre) and into
one that is not; prints msfl_grid_stats of both at the start and at the end, and per checkpoint the median ms per insert of both
and per crop.

--load (with --window): the cost of paging tiles back in.  Two stores are fed the same stream and cropped to the window after every
insert with msfl_grid_crop_tiles.  Whenever a crop evicted something, its tiles are put back at once -- into one store with
msfl_grid_load_cells, into the other with msfl_grid_insert_scan of the same points (the only way back before the load existed) --
both calls timed, in alternating order, and the stores are cropped again (not timed).  Prints per checkpoint and at the end the median
and the 10th / 90th percentile of both, with the median tile size.
"""
import argparse, gc, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from msf_loam_amd import capi


def scan_at(rng, k, n):
    c = np.array([2.0 * k, 0.3 * np.sin(0.05 * k) * 40.0, 0.0])
    p = np.empty((n, 4), np.float32)
    m = n // 2
    p[:m, 0] = rng.uniform(-40, 40, m); p[:m, 1] = rng.uniform(-40, 40, m); p[:m, 2] = rng.normal(0, 0.02, m)       # ground
    p[m:, 0] = rng.uniform(-40, 40, n - m); p[m:, 1] = rng.choice([-12.0, 12.0], n - m) + rng.normal(0, 0.02, n - m)
    p[m:, 2] = rng.uniform(0, 6, n - m)                                                                               # walls
    p[:, :3] += c
    p[:, 3] = 0
    return p, c


def window_leg(a):
    half = [int(v) for v in a.window.split(",")]
    assert len(half) == 3, "--window takes HX,HY,HZ"
    h = capi.Handle()
    stores = {"windowed": capi.Grid(h, 3.0, 0.2), "free": capi.Grid(h, 3.0, 0.2)}
    rngs = {k: np.random.default_rng(7) for k in stores}
    gc.collect(); gc.disable()
    t = {"windowed": [], "free": [], "crop": []}
    for k in range(a.scans):
        for name, g in stores.items():
            p, c = scan_at(rngs[name], k, a.points)
            t0 = time.perf_counter(); g.insert_scan(p); t1 = time.perf_counter()
            t[name].append(t1 - t0)
            if name == "windowed":
                info = g.crop(c, half)
                t["crop"].append(time.perf_counter() - t1)
        if k == 0:
            print(json.dumps({"scans": 1, "stats": {name: g.stats() for name, g in stores.items()}}), flush=True)
        if (k + 1) % a.every == 0:
            print(json.dumps({"scans": k + 1, "window_cells": info.n_cells, "evicted_cells_last_crop": info.n_cells_evicted,
                              **{name + "_ms": round(1e3 * float(np.median(v[-a.every:])), 4) for name, v in t.items()}}), flush=True)
    print(json.dumps({"scans": a.scans, "stats": {name: g.stats() for name, g in stores.items()}}), flush=True)
    for g in stores.values():
        g.close()
    h.close()


def _spread(v):
    v = 1e3 * np.asarray(v, np.float64)
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4), "p90_ms": round(float(np.percentile(v, 90)), 4)}


def load_leg(a):
    half = [int(v) for v in a.window.split(",")]
    assert len(half) == 3, "--window takes HX,HY,HZ"
    h = capi.Handle()
    stores = {"load": capi.Grid(h, 3.0, 0.2), "insert": capi.Grid(h, 3.0, 0.2)}
    rngs = {k: np.random.default_rng(7) for k in stores}
    gc.collect(); gc.disable()
    t = {"load": [], "insert": []}
    tile_pts, tile_cells, n_timed = [], [], 0
    for k in range(a.scans):
        tiles = {}
        for name, g in stores.items():
            p, c = scan_at(rngs[name], k, a.points)
            g.insert_scan(p)
            tiles[name] = g.crop_tiles(c, half)
        if tiles["load"][0].n_cells_evicted > 0 and tiles["insert"][0].n_cells_evicted > 0:
            order = ("load", "insert") if n_timed % 2 == 0 else ("insert", "load")
            n_timed += 1
            for name in order:
                _, cells, pts = tiles[name]
                g = stores[name]
                t0 = time.perf_counter()
                if name == "load":
                    g.load_cells(cells, pts)
                else:
                    g.insert_scan(pts)
                t[name].append(time.perf_counter() - t0)
                g.crop(c, half)                                           # out again, not timed
            tile_pts.append(len(tiles["load"][2])); tile_cells.append(len(tiles["load"][1]))
        if (k + 1) % a.every == 0 and t["load"]:
            m = min(len(t["load"]), a.every)
            print(json.dumps({"scans": k + 1, "tiles_timed": n_timed, "window_cells": stores["load"].size()[1],
                              "load": _spread(t["load"][-m:]), "insert": _spread(t["insert"][-m:])}), flush=True)
    print(json.dumps({"scans": a.scans, "tiles_timed": n_timed, "median_tile_points": float(np.median(tile_pts)) if tile_pts else 0,
                      "median_tile_cells": float(np.median(tile_cells)) if tile_cells else 0,
                      "load": _spread(t["load"]) if t["load"] else None, "insert": _spread(t["insert"]) if t["insert"] else None}), flush=True)
    for g in stores.values():
        g.close()
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1200)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--window", default=None, metavar="HX,HY,HZ", help="the windowed-map leg: insert with and without a crop to this window after every insert")
    ap.add_argument("--load", action="store_true", help="with --window: time msfl_grid_load_cells of every crop's tiles against msfl_grid_insert_scan of the same points")
    a = ap.parse_args()
    if a.load:
        if not a.window:
            ap.error("--load needs --window")
        return load_leg(a)
    if a.window:
        return window_leg(a)
    rng = np.random.default_rng(7)
    h = capi.Handle()
    g = capi.Grid(h, 3.0, 0.2)
    gc.collect(); gc.disable()
    t_ins, t_sur = [], []
    for k in range(a.scans):
        p, c = scan_at(rng, k, a.points)
        t0 = time.perf_counter(); g.insert_scan(p); t1 = time.perf_counter()
        pose = np.array([c[0], c[1], c[2], 0, 0, 0, 1], np.float64)
        q = p.copy(); q[:, :3] -= c
        t2 = time.perf_counter(); out = g.get_surrounded(q, pose); t3 = time.perf_counter()
        t_ins.append(t1 - t0); t_sur.append(t3 - t2)
        if (k + 1) % a.every == 0:
            n, cells = g.size()
            print(json.dumps({"scans": k + 1, "map_points": n, "cells": cells, "surround_points": len(out),
                              "insert_ms": round(1e3 * float(np.median(t_ins[-a.every:])), 4),
                              "surround_ms": round(1e3 * float(np.median(t_sur[-a.every:])), 4)}), flush=True)
    g.close(); h.close()


if __name__ == "__main__":
    main()
