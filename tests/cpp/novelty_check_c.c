/* include/msfl_c_api.h stays a C header: the declarations of msfl_grid_render, msfl_novelty_default_config, msfl_scan_novelty and
   msfl_grids_scan_novelty compile as C99 (tests/test_novelty_declarations.py; compile only). */
#include "msfl_c_api.h"

int novelty_check_c(msfl_handle* h, msfl_grid* corner, msfl_grid* surf, const msfl_point* scan, int n, uint8_t* cls, msfl_point* masked, float* img) {
  msfl_novelty_config cfg;
  msfl_novelty_info info;
  msfl_grid_render_info rinfo;
  msfl_grid* const grids[2] = {corner, surf};
  const double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  msfl_status s;
  msfl_novelty_default_config(&cfg);
  cfg.min_support = 2;
  cfg.keep_classes = (1 << MSFL_NOV_COVERED) | (1 << MSFL_NOV_UNSEEN);
  s = msfl_grid_render(corner, pose, &cfg.image, img, 0, MSFL_MEM_HOST, &rinfo);
  if (s != MSFL_OK) return -1;
  s = msfl_grid_render(surf, pose, &cfg.image, img, 1, MSFL_MEM_HOST, (msfl_grid_render_info*)0);
  if (s != MSFL_OK) return -2;
  s = msfl_scan_novelty(h, scan, n, img, &cfg, cls, masked, &info, MSFL_MEM_HOST);
  if (s != MSFL_OK) return -3;
  s = msfl_grids_scan_novelty(grids, 2, scan, n, pose, &cfg, cls, masked, img, &info, MSFL_MEM_HOST);
  return s == MSFL_OK ? rinfo.n_tested + rinfo.applied + info.n_class[MSFL_NOV_CLASSES - 1] + info.n_map_pixels + info.n_kept + info.applied + info.reserved_
                      : -4;
}
