/* include/msfl_c_api.h stays a C header: the declarations of msfl_grid_load_cells / msfl_grid_crop_tiles compile as C99
   (tests/test_load_declarations.py; compile only). */
#include "msfl_c_api.h"

int load_check_c(msfl_grid* g, const int* cells, int n_cells, const msfl_point* pts, int n_points, int* flags, int* out_cells) {
  msfl_grid_load_info info;
  msfl_grid_crop_info crop;
  const double centre[3] = {0.0, 0.0, 0.0};
  const int half[3] = {1, 1, 1};
  msfl_point ev[4];
  msfl_status s = msfl_grid_load_cells(g, cells, n_cells, pts, n_points, MSFL_MEM_HOST, flags, &info);
  if (s != MSFL_OK) return info.n_conflicts + info.n_bad_points;
  s = msfl_grid_crop_tiles(g, centre, half, ev, 4, out_cells, 1, MSFL_MEM_HOST, &crop);
  return s == MSFL_OK ? info.n_cells_loaded + info.n_points_loaded + info.n_cells + info.n_points + info.applied + info.reserved_ + crop.applied : -1;
}
