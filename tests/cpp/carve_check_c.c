/* include/msfl_c_api.h stays a C header: the declarations of msfl_grid_carve, msfl_carve_tables and msfl_carve_default_config compile
   as C99 (tests/test_carve_declarations.py; compile only). */
#include "msfl_c_api.h"

int carve_check_c(msfl_grid* g, const msfl_point* scan, int n, msfl_point* removed, int capacity) {
  msfl_carve_config cfg;
  msfl_grid_carve_info info;
  const double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  float cc[360], cs[360], ec[17], es[17];
  msfl_status s;
  msfl_carve_default_config(&cfg);
  cfg.window_col = 2;
  s = msfl_carve_tables(&cfg, cc, cs, ec, es);
  if (s != MSFL_OK) return -1;
  s = msfl_grid_carve(g, scan, n, pose, &cfg, removed, capacity, MSFL_MEM_HOST, &info);
  return s == MSFL_OK ? info.n_points_removed + info.n_cells_emptied + info.n_cells + info.n_points + info.n_tested + info.n_pixels + info.applied +
                            info.reserved_
                      : -2;
}
