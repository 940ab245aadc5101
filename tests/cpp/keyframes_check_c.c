/* include/msfl_c_api.h stays a C header: the declarations of msfl_keyframes_* compile as C99
   (tests/test_keyframes_model.py; compile only). */
#include "msfl_c_api.h"

int keyframes_check_c(msfl_handle* h, msfl_grid* gc, msfl_grid* gs, const msfl_point* pts, const int* idx, int n) {
  msfl_keyframes_config cfg;
  msfl_keyframes* k = 0;
  int index = -1, n_corner = 0, n_surf = 0, n_done = 0;
  const int member_off[2] = {0, 1};
  const int keys[1] = {0};
  const double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  int off_c[2], off_s[2];
  msfl_point out_c[8], out_s[8];
  msfl_status s;
  msfl_keyframes_default_config(&cfg);
  cfg.leaf_corner = 0.0f;
  s = msfl_keyframes_create(h, &cfg, &k);
  if (s != MSFL_OK) return -1;
  s = msfl_keyframes_add(k, pts, idx, n, pts, 0, n, MSFL_MEM_HOST, &index);
  if (s == MSFL_OK) s = msfl_keyframes_sizes(k, index, 1, &n_corner, &n_surf);
  if (s == MSFL_OK) s = msfl_keyframes_get(k, index, out_c, 8, out_s, 8, MSFL_MEM_HOST);
  if (s == MSFL_OK)
    s = msfl_keyframes_compose(k, 1, member_off, keys, pose, 0.0f, cfg.leaf_surf, out_c, 8, off_c, out_s, 8, off_s, MSFL_MEM_HOST);
  if (s == MSFL_OK) s = msfl_keyframes_insert(k, keys, pose, 1, gc, gs, &n_done);
  n = msfl_keyframes_size(k) + cfg.max_keyframes + cfg.max_corner_points + cfg.max_surf_points;
  msfl_keyframes_destroy(k);
  return s == MSFL_OK ? n + n_corner + n_surf + n_done + off_c[1] + off_s[1] : -(int)s;
}
