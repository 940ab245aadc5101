// The record buffer's index arithmetic (msf_loam_amd/csrc/msfl_record_tiles.h) through plain g++, for tests/test_record_tiles_model.py.
// usage: record_tiles_check <n_corner_total> <n_surf_total>
// prints "layout <plane region doubles> <buffer doubles> <reserved doubles>", then per plane slot g
//        "slot g <xy> <zc> <elem 0..3> <nn4 byte> <nn1 byte>" (offsets in doubles unless named bytes), then per edge slot "edge e <offset>".
#include <cstdio>
#include <cstdlib>

#include "msfl_record_tiles.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const size_t nc = (size_t)std::atol(argv[1]), ns = (size_t)std::atol(argv[2]);
  std::printf("layout %zu %zu %zu\n", rec_plane_region(ns), rec_buffer_doubles(nc, ns), rec_reserve_doubles(nc + ns, ns));
  for (size_t g = 0; g < ns; g++)
    std::printf("slot %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", g, rec_tile_xy(g), rec_tile_zc(g), rec_tile_elem(g, 0), rec_tile_elem(g, 1),
                rec_tile_elem(g, 2), rec_tile_elem(g, 3), rec_tile_nn4(g), rec_tile_nn1(g));
  for (size_t e = 0; e < nc; e++) std::printf("edge %zu %zu\n", e, rec_edge(ns, e));
  return 0;
}
