// Layout of the record buffer (index arithmetic only: compiles as plain C++, tests/cpp/record_tiles_check.cpp).
//
// PLANE records {N.x, N.y, N.z, N.C} of the whole batch come first, in lane-transposed tiles of 64 rows: plane slot g (the surf
// feature's index in its cloud minus the batch's first) belongs to tile g >> 6 at lane g & 63.  A tile is 2 048 bytes: its first
// half holds {N.x, N.y} of the 64 lanes, its second half {N.z, N.C}.  A wavefront that reads or writes 64 consecutive rows therefore
// issues two accesses of 1 KB contiguous each (a scan that starts mid-tile: two contiguous pieces each) instead of two accesses at
// a 32-byte lane stride that touch the same 16 lines twice.  The plane region is padded to whole tiles; the EDGE records
// {C, N} (6 doubles each, gathered through the index list) follow it unchanged.
//
// On the whole-batch path the 5-NN list of a surf feature lives in the tile its record will occupy (knn5_scan2map_split_kernel ->
// fit_scan2map_split_kernel): {p0..p3} of lane l at byte 16 l of the tile, p4 at byte 1024 + 4 l.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MSFL_TILE_FN __host__ __device__ __forceinline__
#else
#define MSFL_TILE_FN inline
#endif

enum { kRecTileRows = 64, kRecTileDoubles = 256, kRecTileBytes = 2048 };

// offsets in doubles from the start of the record buffer
MSFL_TILE_FN size_t rec_tile_xy(size_t g) { return (g >> 6) * kRecTileDoubles + 2 * (g & 63); }     // {N.x, N.y} of plane slot g
MSFL_TILE_FN size_t rec_tile_zc(size_t g) { return rec_tile_xy(g) + kRecTileDoubles / 2; }           // {N.z, N.C}
MSFL_TILE_FN size_t rec_tile_elem(size_t g, int k) { return rec_tile_xy(g) + (size_t)(k & 1) + (size_t)(k >> 1) * (kRecTileDoubles / 2); }   // element k of the row
MSFL_TILE_FN size_t rec_plane_region(size_t n_surf_total) { return kRecTileDoubles * ((n_surf_total + 63) >> 6); }   // = start of the edge region
MSFL_TILE_FN size_t rec_edge(size_t n_surf_total, size_t e) { return rec_plane_region(n_surf_total) + 6 * e; }     // edge slot e
MSFL_TILE_FN size_t rec_buffer_doubles(size_t n_corner_total, size_t n_surf_total) { return rec_edge(n_surf_total, n_corner_total); }
// what the host reserves for a batch of n_rec records, n_surf_total of them planes: 6 doubles per record as ever, which holds the layout
// for all but the smallest batches (the tile padding is < 256 doubles); those get the layout's size
MSFL_TILE_FN size_t rec_reserve_doubles(size_t n_rec, size_t n_surf_total) {
  const size_t flat = 6 * (n_rec > 0 ? n_rec : 1), tiled = rec_buffer_doubles(n_rec - n_surf_total, n_surf_total);
  return flat > tiled ? flat : tiled;
}
// offsets in BYTES of the neighbour list of plane slot g while its tile holds lists
MSFL_TILE_FN size_t rec_tile_nn4(size_t g) { return (g >> 6) * kRecTileBytes + 16 * (g & 63); }      // int4 {p0, p1, p2, p3}
MSFL_TILE_FN size_t rec_tile_nn1(size_t g) { return (g >> 6) * kRecTileBytes + 1024 + 4 * (g & 63); }   // int p4
