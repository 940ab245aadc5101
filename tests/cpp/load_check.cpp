// Tiles through the C++ mirror (include/msfl/scan_matcher.hpp): HybridGrid::CropTiles delivers the evicted cells and their points,
// HybridGrid::LoadCells takes the pair back, and the same crop run again delivers the same bytes.  Also names every new C
// declaration of include/msfl_c_api.h, so that compiling this file checks them (tests/test_load_declarations.py compiles it on the
// CPU and runs it on the GPU; tests/cpp/Makefile does not know it).  Exit status 0: all checks hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "msfl/scan_matcher.hpp"

static_assert(sizeof(msfl_grid_load_info) == 8 * sizeof(int), "msfl_grid_load_info is 8 ints");
static msfl_status (*const kLoad)(msfl_grid*, const int*, int, const msfl_point*, int, msfl_mem, int*, msfl_grid_load_info*) = &msfl_grid_load_cells;
static msfl_status (*const kCropTiles)(msfl_grid*, const double[3], const int[3], msfl_point*, int, int*, int, msfl_mem, msfl_grid_crop_info*) =
    &msfl_grid_crop_tiles;

static int fail(const char* what) { std::fprintf(stderr, "load_check: %s\n", what); return 1; }

int main() {
  (void)kLoad; (void)kCropTiles;
  auto cloud = std::make_shared<msfl::PointCloud<msfl::PointType>>();
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  for (int i = 0; i < 600; ++i) {                           // 12 cells along x, 50 points each on a 0.05 m lattice
    float p[4] = {0.3f + 3.0f * static_cast<float>(i / 50) + 0.05f * static_cast<float>(i % 7), 0.1f * static_cast<float>(i % 11) - 0.5f,
                  0.07f * static_cast<float>(i % 5), 0.001f * static_cast<float>(i)};
    msfl::PointType q;
    std::memcpy(&q, p, 16);
    cloud->points.push_back(q);
  }
  msfl::HybridGrid grid(3.0f, 0.4f, 0);
  grid.InsertScan(cloud);
  const std::array<double, 3> centre = {{3.2, 0.0, 0.0}};
  const std::array<int, 3> half = {{1, 1, 1}};
  std::vector<msfl_point> ev1, ev2;
  std::vector<int> cells1, cells2, conflict;
  const msfl_grid_crop_info c1 = grid.CropTiles(centre, half, &ev1, &cells1);
  if (!(c1.applied == 1 && c1.n_cells_evicted == 9 && c1.n_cells == 3 && cells1.size() == 36 && static_cast<int>(ev1.size()) == c1.n_points_evicted))
    return fail("the first crop");
  const msfl_grid_load_info l = grid.LoadCells(cells1, ev1, &conflict);
  if (!(l.applied == 1 && l.n_cells_loaded == 9 && l.n_points_loaded == c1.n_points_evicted && l.n_cells == 12 &&
        l.n_points == c1.n_points + c1.n_points_evicted && l.n_conflicts == 0 && l.n_bad_points == 0 && conflict == std::vector<int>(9, 0)))
    return fail("the load");
  bool thrown = false;
  try { grid.LoadCells(cells1, ev1, &conflict); } catch (const std::exception&) { thrown = true; }       // every listed cell is live now
  if (!thrown || conflict != std::vector<int>(9, 1)) return fail("the refused load");
  const msfl_grid_crop_info c2 = grid.CropTiles(centre, half, &ev2, &cells2);
  if (std::memcmp(&c1, &c2, sizeof(c1)) != 0 || cells1 != cells2 || ev1.size() != ev2.size() ||
      std::memcmp(ev1.data(), ev2.data(), ev1.size() * sizeof(msfl_point)) != 0)
    return fail("the second crop differs from the first");
  std::printf("load_check ok: %d cells, %d points\n", c1.n_cells_evicted, c1.n_points_evicted);
  return 0;
}
