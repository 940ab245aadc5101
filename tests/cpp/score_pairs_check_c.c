/* include/msfl_c_api.h stays a C header with the resident pair maps in it: the declarations of msfl_set_pair_maps,
   msfl_score_pairs and msfl_match_pairs_resident compile as C99 and have exactly these prototypes
   (tests/test_score_pairs_model.py; compile only). */
#include "msfl_c_api.h"

typedef msfl_status (*set_pair_maps_fn)(msfl_handle*, int, const msfl_point*, const int*, const msfl_point*, const int*, msfl_mem);
typedef msfl_status (*score_pairs_fn)(msfl_handle*, int, const msfl_point*, const int*, const msfl_point*, const int*, const double*,
                                      const int*, double, msfl_pose_score*, float*, int*, msfl_mem);
typedef msfl_status (*match_pairs_resident_fn)(msfl_handle*, int, const msfl_point*, const int*, const msfl_point*, const int*, double*,
                                               int*, msfl_match_info*, msfl_mem);

int score_pairs_check_c(msfl_handle* h, const msfl_point* map_corner, int n_map_corner, const msfl_point* map_surf, int n_map_surf,
                        const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf, double* pose, msfl_pose_score* score) {
  const set_pair_maps_fn set_maps = &msfl_set_pair_maps;
  const score_pairs_fn score_pairs = &msfl_score_pairs;
  const match_pairs_resident_fn match = &msfl_match_pairs_resident;
  int mco[2], mso[2], co[2], so[2], po[2], status = 0;
  msfl_status s;
  mco[0] = 0; mco[1] = n_map_corner; mso[0] = 0; mso[1] = n_map_surf;
  co[0] = 0; co[1] = n_corner; so[0] = 0; so[1] = n_surf; po[0] = 0; po[1] = 1;
  s = set_maps(h, 1, map_corner, mco, map_surf, mso, MSFL_MEM_HOST);
  if (s != MSFL_OK) return -1;
  s = match(h, 1, corner, co, surf, so, pose, &status, 0, MSFL_MEM_HOST);
  if (s != MSFL_OK || status != MSFL_OK) return -1;
  s = score_pairs(h, 1, corner, co, surf, so, pose, po, 1.0, score, 0, 0, MSFL_MEM_HOST);
  return s == MSFL_OK ? score[0].inliers[0] + score[0].inliers[1] : -1;
}
