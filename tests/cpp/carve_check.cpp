// HybridGrid::Carve through the C++ mirror (include/msfl/scan_matcher.hpp): a wall of stored points 10 m ahead, a blob 5 m ahead,
// and a scan that returns the wall.  The blob goes and is delivered, the wall stays, a second carve removes nothing.  Also names the
// new C declarations of include/msfl_c_api.h, so that compiling this file checks them (tests/test_carve_declarations.py compiles it
// on the CPU and runs it on the GPU).  Exit status 0: all checks hold.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "msfl/scan_matcher.hpp"

static_assert(sizeof(msfl_grid_carve_info) == 8 * sizeof(int), "msfl_grid_carve_info is 8 ints");
static_assert(sizeof(msfl_carve_config) == 10 * sizeof(int), "msfl_carve_config is 10 words");
static msfl_status (*const kCarve)(msfl_grid*, const msfl_point*, int, const double[7], const msfl_carve_config*, msfl_point*, int, msfl_mem,
                                   msfl_grid_carve_info*) = &msfl_grid_carve;
static msfl_status (*const kTables)(const msfl_carve_config*, float*, float*, float*, float*) = &msfl_carve_tables;
static void (*const kDefaults)(msfl_carve_config*) = &msfl_carve_default_config;

static int fail(const char* what) { std::fprintf(stderr, "carve_check: %s\n", what); return 1; }

static msfl::PointType point(double x, double y, double z, float w) {
  const float p[4] = {static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), w};
  msfl::PointType q;
  std::memcpy(&q, p, 16);
  return q;
}

int main() {
  (void)kCarve; (void)kTables; (void)kDefaults;
  const double kDeg = 3.14159265358979323846 / 180.0;
  auto stored = std::make_shared<msfl::PointCloud<msfl::PointType>>();
  auto scan = std::make_shared<msfl::PointCloud<msfl::PointType>>();
  for (int j = -4; j <= 4; ++j)
    for (int k = -1; k <= 1; ++k) stored->points.push_back(point(10.0, 0.8 * j, 0.8 * k + 0.1, 1.0f));      // the wall: 27 points
  for (int j = -1; j <= 1; ++j) stored->points.push_back(point(5.0, 0.8 * j, 0.1, 2.0f));                    // the blob: 3 points
  for (int col = -80; col < 80; ++col)                                                                     // the scan: the wall, every pixel's centre
    for (int beam = 0; beam < 16; ++beam) {
      const double az = (col + 0.5) * 0.5 * kDeg, el = (-15.0 + 2.0 * beam) * kDeg, r = 10.0 / (std::cos(az) * std::cos(el));
      scan->points.push_back(point(r * std::cos(el) * std::cos(az), r * std::cos(el) * std::sin(az), r * std::sin(el), 0.0f));
    }
  msfl::HybridGrid grid(3.0f, 0.4f, 0);
  grid.InsertScan(stored);
  std::vector<msfl_point> removed;
  const msfl_grid_carve_info a = grid.Carve(scan, msfl::Rigid3d::Identity(), nullptr, &removed);
  if (!(a.applied == 1 && a.n_points_removed == 3 && removed.size() == 3 && a.n_points == 27 && a.n_tested == 30 && a.n_pixels == 160 * 16))
    return fail("the first carve");
  for (const msfl_point& p : removed) if (p.x != 5.0f) return fail("the removed points");
  msfl_carve_config cfg;
  msfl_carve_default_config(&cfg);
  cfg.window_col = 0;
  const msfl_grid_carve_info b = grid.Carve(scan, msfl::Rigid3d::Identity(), &cfg);
  if (!(b.applied == 1 && b.n_points_removed == 0 && b.n_points == 27 && b.n_cells == a.n_cells)) return fail("the second carve");
  std::printf("carve_check ok: %d removed, %d left\n", a.n_points_removed, b.n_points);
  return 0;
}
