/* include/msfl_c_api.h stays a C header: the records of the pose search have the sizes the bindings assume and the declarations of
   msfl_search_default_config, msfl_search_geometry, msfl_search_poses and msfl_relocalize compile as C99.  search_check_c runs the
   four through function pointers of the declared types (tests/test_search_model.py compiles it; tests/test_gpu_search.py links
   and runs it). */
#include "msfl_c_api.h"

typedef char msfl_search_config_is_72_bytes[sizeof(msfl_search_config) == 72 ? 1 : -1];
typedef char msfl_search_geom_is_72_bytes[sizeof(msfl_search_geom) == 72 ? 1 : -1];
typedef char msfl_pose_candidate_is_88_bytes[sizeof(msfl_pose_candidate) == 88 ? 1 : -1];
typedef char msfl_reloc_result_is_216_bytes[sizeof(msfl_reloc_result) == 216 ? 1 : -1];

typedef void (*default_fn)(msfl_search_config*);
typedef msfl_status (*geometry_fn)(const double*, const msfl_search_config*, int, int, msfl_search_geom*);
typedef msfl_status (*search_fn)(msfl_handle*, const msfl_point*, int, const msfl_point*, int, const double*, const msfl_search_config*,
                                 msfl_pose_candidate*, int, int*, int*, msfl_mem);
typedef msfl_status (*relocalize_fn)(msfl_handle*, const msfl_point*, int, const msfl_point*, int, const double*, const msfl_search_config*, int,
                                     double, int, double, msfl_reloc_result*, int, int*, msfl_mem);

/* The handle already holds a map.  cfg: null = the defaults.  Returns the candidates written, or -1 - status of the call that failed. */
int search_check_c(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf, const double* guess,
                   const msfl_search_config* cfg, msfl_pose_candidate* candidates, int capacity, int* hits_out, msfl_reloc_result* results,
                   int n_refine, int* n_results) {
  const default_fn defaults = &msfl_search_default_config;
  const geometry_fn geometry = &msfl_search_geometry;
  const search_fn search = &msfl_search_poses;
  const relocalize_fn relocalize = &msfl_relocalize;
  msfl_search_config c;
  msfl_search_geom g;
  msfl_status s;
  int n = 0;
  defaults(&c);
  if (cfg) c = *cfg;
  s = geometry(guess, &c, n_corner, n_surf, &g);
  if (s != MSFL_OK) return -1 - (int)s;
  s = search(h, corner, n_corner, surf, n_surf, guess, &c, candidates, capacity, &n, hits_out, MSFL_MEM_HOST);
  if (s != MSFL_OK) return -1 - (int)s;
  s = relocalize(h, corner, n_corner, surf, n_surf, guess, &c, capacity, 1.0, n_refine, 0.5, results, n_refine, n_results, MSFL_MEM_HOST);
  if (s != MSFL_OK) return -1 - (int)s;
  return n;
}
