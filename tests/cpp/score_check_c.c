/* include/msfl_c_api.h stays a C header: msfl_pose_score is 32 bytes and the declarations of msfl_score_poses /
   msfl_score_poses_batch compile as C99 (tests/test_score_model.py; compile only). */
#include "msfl_c_api.h"

typedef char msfl_pose_score_is_32_bytes[sizeof(msfl_pose_score) == 32 ? 1 : -1];

typedef msfl_status (*score_fn)(msfl_handle*, const msfl_point*, int, const msfl_point*, int, const double*, int, double, msfl_pose_score*,
                                float*, int*, msfl_mem);
typedef msfl_status (*score_batch_fn)(msfl_handle*, int, const msfl_point*, const int*, const msfl_point*, const int*, const double*,
                                      const int*, double, msfl_pose_score*, msfl_mem);

int score_check_c(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf, const double* poses, int n_poses,
                  msfl_pose_score* scores) {
  const score_fn one = &msfl_score_poses;
  const score_batch_fn many = &msfl_score_poses_batch;
  int co[2], so[2], po[2];
  msfl_status s;
  co[0] = 0; co[1] = n_corner; so[0] = 0; so[1] = n_surf; po[0] = 0; po[1] = n_poses;
  s = one(h, corner, n_corner, surf, n_surf, poses, n_poses, 1.0, scores, 0, 0, MSFL_MEM_HOST);
  if (s != MSFL_OK) return -1;
  s = many(h, 1, corner, co, surf, so, poses, po, 1.0, scores, MSFL_MEM_HOST);
  return s == MSFL_OK ? scores[0].inliers[0] + scores[0].inliers[1] + (int)(scores[0].sum_sq_q32[0] & 1u) + scores[0].status + scores[0].reserved_ : -1;
}
