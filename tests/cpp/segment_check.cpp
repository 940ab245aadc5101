// ScanRegistration::Segment through the C++ mirror (include/msfl/scan_matcher.hpp): level ground under the four downward beams of
// every column, a wall patch of 6 columns x 8 upward beams at 10 m and one stray return.  The ground is GROUND, the patch one
// SEGMENT, the stray an OUTLIER that the masked cloud drops.  Also names the new C declarations of include/msfl_c_api.h, so that
// compiling this file checks them (tests/test_segment_declarations.py compiles it on the CPU and runs it on the GPU).  Exit status 0:
// all checks hold.
#include <cmath>
#include <cstdio>
#include <vector>

#include "msfl/scan_matcher.hpp"

static_assert(sizeof(msfl_segment_info) == 10 * sizeof(int), "msfl_segment_info is 10 ints");
static_assert(sizeof(msfl_segment_config) == 72, "msfl_segment_config is 72 bytes");
static msfl_status (*const kScans)(msfl_handle*, int, const msfl_point*, const uint16_t*, const int*, const msfl_segment_config*, uint8_t*, int*,
                                   msfl_point*, msfl_segment_info*, msfl_mem) = &msfl_segment_scans;
static msfl_status (*const kScan)(msfl_handle*, const msfl_point*, const uint16_t*, int, const msfl_segment_config*, uint8_t*, int*, msfl_point*,
                                  msfl_segment_info*, msfl_mem) = &msfl_segment_scan;
static msfl_status (*const kTables)(const msfl_segment_config*, float*, float*, float*, float*, float[4]) = &msfl_segment_tables;
static void (*const kDefaults)(msfl_segment_config*) = &msfl_segment_default_config;

static int fail(const char* what) { std::fprintf(stderr, "segment_check: %s\n", what); return 1; }

int main() {
  (void)kScans; (void)kScan; (void)kTables; (void)kDefaults;
  const double kDeg = 3.14159265358979323846 / 180.0;
  msfl::PointCloud<msfl::PointTypeOriginal> cloud;
  auto put = [&](int col, int beam, double r) {
    const double az = col * 0.2 * kDeg, el = (-15.0 + 2.0 * beam) * kDeg;
    msfl::PointTypeOriginal p{};
    p.x = static_cast<float>(r * std::cos(el) * std::cos(az)); p.y = static_cast<float>(r * std::cos(el) * std::sin(az));
    p.z = static_cast<float>(r * std::sin(el)); p.intensity = 0.25f; p.ring = static_cast<std::uint16_t>(beam); p.time = 0.25f;
    cloud.push_back(p);
  };
  for (int col = 0; col < 1800; ++col)
    for (int beam = 0; beam < 4; ++beam) put(col, beam, 1.8 / -std::sin((-15.0 + 2.0 * beam) * kDeg));      // 7 200 ground returns
  for (int col = 100; col < 106; ++col)
    for (int beam = 8; beam < 16; ++beam) put(col, beam, 10.0);                                              // 48 on the patch
  put(900, 12, 30.0);                                                                                        // the stray
  msfl::ScanRegistration reg(0);
  std::vector<std::uint8_t> cls;
  msfl::PointCloud<msfl::PointTypeOriginal> masked;
  const msfl_segment_info a = reg.Segment(cloud, &cls, &masked);
  if (!(a.n_class[MSFL_SEG_GROUND] == 7200 && a.n_class[MSFL_SEG_SEGMENT] == 48 && a.n_class[MSFL_SEG_OUTLIER] == 1 && a.n_class[MSFL_SEG_NONE] == 0 &&
        a.n_class[MSFL_SEG_SHADOWED] == 0 && a.n_pixels == 7249 && a.n_components == 2 && a.n_segments == 1 && a.n_kept == 7248))
    return fail("the counts");
  if (cls.size() != cloud.size() || masked.size() != cloud.size()) return fail("the sizes");
  for (std::size_t i = 0; i < cloud.size(); ++i) {
    const bool kept = cls[i] == MSFL_SEG_GROUND || cls[i] == MSFL_SEG_SEGMENT;
    if (kept != (i + 1 < cloud.size())) return fail("the classes");
    if (kept ? (masked[i].x != cloud[i].x || masked[i].z != cloud[i].z) : !(std::isnan(masked[i].x) && std::isnan(masked[i].y) && std::isnan(masked[i].z)))
      return fail("the masked cloud");
    if (masked[i].ring != cloud[i].ring || masked[i].intensity != 0.25f) return fail("the fields the mask leaves alone");
  }
  msfl_segment_config cfg;
  msfl_segment_default_config(&cfg);
  cfg.keep_classes = 1 << MSFL_SEG_OUTLIER;
  cfg.min_points = 49;                                                                                       // the patch is tall, so it stays valid
  const msfl_segment_info b = reg.Segment(cloud, nullptr, nullptr, &cfg);
  if (!(b.n_kept == 1 && b.n_segments == 1)) return fail("the second call");
  const auto scan = reg.Extract(masked, 0.0);                                                                // NaN points go in the invalid-point pass
  if (scan.cloud_full_res->size() != 7248) return fail("extraction of the masked cloud");
  std::printf("segment_check ok: %d ground, %d segment, %d outlier\n", a.n_class[MSFL_SEG_GROUND], a.n_class[MSFL_SEG_SEGMENT], a.n_class[MSFL_SEG_OUTLIER]);
  return 0;
}
