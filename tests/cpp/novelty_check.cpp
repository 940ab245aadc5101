// HybridGrid::Render and ScanNovelty through the C++ mirror (include/msfl/scan_matcher.hpp) on the dense-wall scene of
// tests/novelty_cases.py, at the identity pose: a 36 x 4 image, one stored point at the centre direction of every pixel 10 m away
// except in columns 14 .. 20, and a scan of the same directions at 10 m (covered), a patch at 4 m (in front) and the directions of
// columns 16 .. 18 at 6 m (unseen).  Also names the new C declarations of include/msfl_c_api.h, so that compiling this file checks
// them (tests/test_novelty_declarations.py compiles it on the CPU and runs it on the GPU).  Exit status 0: all checks hold.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "msfl/scan_matcher.hpp"

static_assert(sizeof(msfl_grid_render_info) == 2 * sizeof(int), "msfl_grid_render_info is 2 ints");
static_assert(sizeof(msfl_novelty_info) == 8 * sizeof(int), "msfl_novelty_info is 8 ints");
static_assert(sizeof(msfl_novelty_config) == sizeof(msfl_carve_config) + 2 * sizeof(int), "msfl_novelty_config is the image and 2 ints");
static_assert(MSFL_NOV_NONE == 0 && MSFL_NOV_UNSEEN == 1 && MSFL_NOV_COVERED == 2 && MSFL_NOV_IN_FRONT == 3 && MSFL_NOV_CLASSES == 4, "the classes");
static msfl_status (*const kRender)(msfl_grid*, const double[7], const msfl_carve_config*, float*, int, msfl_mem, msfl_grid_render_info*) = &msfl_grid_render;
static void (*const kDefaults)(msfl_novelty_config*) = &msfl_novelty_default_config;
static msfl_status (*const kLabel)(msfl_handle*, const msfl_point*, int, const float*, const msfl_novelty_config*, uint8_t*, msfl_point*, msfl_novelty_info*,
                                   msfl_mem) = &msfl_scan_novelty;
static msfl_status (*const kChain)(msfl_grid* const*, int, const msfl_point*, int, const double[7], const msfl_novelty_config*, uint8_t*, msfl_point*, float*,
                                   msfl_novelty_info*, msfl_mem) = &msfl_grids_scan_novelty;

static int fail(const char* what) { std::fprintf(stderr, "novelty_check: %s\n", what); return 1; }

static msfl::PointType ray(int col, int row, double r, float w) {
  const double kDeg = 3.14159265358979323846 / 180.0;
  const double az = (col + 0.5) * 10.0 * kDeg, el = (-16.0 + (row + 0.5) * 8.0) * kDeg;
  const float p[4] = {static_cast<float>(r * std::cos(el) * std::cos(az)), static_cast<float>(r * std::cos(el) * std::sin(az)),
                      static_cast<float>(r * std::sin(el)), w};
  msfl::PointType q;
  std::memcpy(&q, p, 16);
  return q;
}

int main() {
  (void)kRender; (void)kDefaults; (void)kLabel; (void)kChain;
  auto stored = std::make_shared<msfl::PointCloud<msfl::PointType>>();
  auto scan = std::make_shared<msfl::PointCloud<msfl::PointType>>();
  for (int row = 0; row < 4; ++row)
    for (int col = 0; col < 36; ++col)
      if (col < 14 || col > 20) { stored->points.push_back(ray(col, row, 10.0, 1.0f)); scan->points.push_back(ray(col, row, 10.0, 0.0f)); }
  for (int row = 1; row < 3; ++row)
    for (int col = 2; col < 6; ++col) scan->points.push_back(ray(col, row, 4.0, 0.0f));
  for (int row = 0; row < 4; ++row)
    for (int col = 16; col < 19; ++col) scan->points.push_back(ray(col, row, 6.0, 0.0f));
  msfl::HybridGrid grid(3.0f, 0.2f, 0);
  grid.InsertScan(stored);
  msfl_novelty_config cfg;
  msfl_novelty_default_config(&cfg);
  cfg.image.n_col = 36; cfg.image.n_row = 4;
  std::vector<float> image;
  const msfl_grid_render_info r = grid.Render(msfl::Rigid3d::Identity(), &image, &cfg.image);
  if (!(r.applied == 1 && r.n_tested == 116 && image.size() == 36 * 4)) return fail("the render");
  for (int row = 0; row < 4; ++row)
    for (int col = 0; col < 36; ++col) {
      const float v = image[static_cast<std::size_t>(row * 36 + col)];
      if (col < 14 || col > 20 ? !(std::fabs(v - 10.0f) < 1e-3f) : !std::isinf(v)) return fail("the image");
    }
  const msfl::ScanNoveltyResult a = msfl::ScanNovelty({&grid}, scan, msfl::Rigid3d::Identity(), &cfg);
  const int* n = a.info.n_class;
  if (!(a.info.applied == 1 && n[0] == 0 && n[1] == 12 && n[2] == 116 && n[3] == 8 && a.info.n_map_pixels == 116 && a.info.n_kept == 128 &&
        a.kept->points.size() == 128 && a.cls.size() == 136))
    return fail("the labels");
  for (std::size_t i = 0; i < a.cls.size(); ++i)
    if (a.cls[i] != (i < 116 ? MSFL_NOV_COVERED : i < 124 ? MSFL_NOV_IN_FRONT : MSFL_NOV_UNSEEN)) return fail("a point's class");
  cfg.image.window_col = 0;                                  // the narrowest window: the same classes
  const msfl::ScanNoveltyResult b = msfl::ScanNovelty({&grid, &grid}, scan, msfl::Rigid3d::Identity(), &cfg);
  if (b.cls != a.cls) return fail("the narrow window");
  std::printf("novelty_check ok: %d none, %d unseen, %d covered, %d in front\n", n[0], n[1], n[2], n[3]);
  return 0;
}
