/* include/msfl_c_api.h stays a C header: the declarations of msfl_segment_scans, msfl_segment_scan, msfl_segment_tables and
   msfl_segment_default_config compile as C99 (tests/test_segment_declarations.py; compile only). */
#include "msfl_c_api.h"

int segment_check_c(msfl_handle* h, const msfl_point* pts, const uint16_t* ring, const int* off, int n_scans, uint8_t* cls, int* seg,
                    msfl_point* masked, msfl_segment_info* info) {
  msfl_segment_config cfg;
  float cc[900], cs[900], vs[15], vc[15], scalars[4];
  msfl_status s;
  msfl_segment_default_config(&cfg);
  cfg.keep_classes = (1 << MSFL_SEG_GROUND) | (1 << MSFL_SEG_SEGMENT) | (1 << MSFL_SEG_OUTLIER);
  s = msfl_segment_tables(&cfg, cc, cs, vs, vc, scalars);
  if (s != MSFL_OK) return -1;
  s = msfl_segment_scans(h, n_scans, pts, ring, off, &cfg, cls, seg, masked, info, MSFL_MEM_HOST);
  if (s != MSFL_OK) return -2;
  s = msfl_segment_scan(h, pts, ring, off[1] - off[0], &cfg, cls, seg, masked, info, MSFL_MEM_HOST);
  return s == MSFL_OK ? info[0].n_class[MSFL_SEG_NONE] + info[0].n_class[MSFL_SEG_CLASSES - 1] + info[0].n_pixels + info[0].n_components +
                            info[0].n_segments + info[0].n_kept + info[0].reserved_
                      : -3;
}
